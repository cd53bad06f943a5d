"""C ABI of the parameter-free activation kernels (csrc/neuron.hip): symbols, prototypes against the header, the mode constants and the
host-side refusals (no GPU: every call here returns before anything touches a device)."""
import ctypes as C
import os
import re

from conftest import ROOT
from fcn_object_detector_amd import lib as L

E_ARG, E_ALIGN = 1, 2
NAMES = ("fcn_neuron_fwd_f32", "fcn_neuron_fwd_f16", "fcn_neuron_bwd_f32")
X, Y, K = 0x100000, 0x200000, 0x300000      # fake, never dereferenced, 16-byte aligned
NAN = float("nan")


def header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fcnhip.h")).read(), flags=re.S)


def test_symbols_are_exported_and_bound_and_the_abi_version_stays():
    lib = L.load()
    for n in NAMES:
        assert hasattr(lib, n) and n in L.PROTOTYPES, n
    assert lib.fcn_abi_version() == 2


def test_prototypes_and_modes_match_the_header():
    txt = header()
    kinds = {"int": C.c_int, "float": C.c_float, "fcn_stream_t": C.c_void_p}
    for n in NAMES:
        m = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % n, txt, flags=re.S)
        assert m, n
        want = []
        for arg in m.group(1).split(","):
            arg = " ".join(arg.split())
            want.append(C.c_void_p if "*" in arg else kinds[arg.rsplit(" ", 1)[0].replace("const ", "")])
        res, args = L.PROTOTYPES[n]
        assert res is C.c_int and list(args) == want, n
    m = re.search(r"enum\s*\{\s*FCN_NEURON_ELU\s*=\s*(\d+)\s*,\s*FCN_NEURON_CLIP\s*=\s*(\d+)\s*,\s*FCN_NEURON_ABSVAL\s*=\s*(\d+)\s*,"
                  r"\s*FCN_NEURON_BNLL\s*=\s*(\d+)\s*,\s*FCN_NEURON_SWISH\s*=\s*(\d+)\s*\}", txt)
    assert m and tuple(int(v) for v in m.groups()) == (0, 1, 2, 3, 4) == (L.NEURON_ELU, L.NEURON_CLIP, L.NEURON_ABSVAL, L.NEURON_BNLL, L.NEURON_SWISH)
    assert L.NEURON_MODES == {"ELU": 0, "ReLU6": 1, "Clip": 1, "AbsVal": 2, "BNLL": 3, "Swish": 4}
    # the argument names the engines rely on, in order
    order = lambda n: [a.split()[-1].lstrip("*") for a in re.search(r"\b%s\s*\((.*?)\)" % n, txt, flags=re.S).group(1).split(",")]
    assert order(NAMES[0]) == ["x", "y", "keep", "pixels", "C", "x_cstride", "x_coffset", "y_cstride", "y_coffset", "keep_cstride", "mode", "a", "b", "s"]
    assert order(NAMES[1]) == [a for a in order(NAMES[0]) if not a.startswith("keep")]
    assert order(NAMES[2]) == ["dy", "ref", "dx", "pixels", "C", "dy_cstride", "dy_coffset", "ref_cstride", "ref_coffset", "dx_cstride", "dx_coffset",
                               "mode", "a", "b", "accumulate", "s"]


def test_the_act_entry_points_gained_no_mode():
    txt = header()
    assert re.search(r"enum\s*\{\s*FCN_ACT_PRELU\s*=\s*0\s*,\s*FCN_ACT_TANH\s*=\s*1\s*,\s*FCN_ACT_BIAS\s*=\s*2\s*\}", txt)
    assert L.load().fcn_act_fwd_f32(X, Y, None, 5, 8, 16, 0, 16, 0, 0, 3, None, 0, None) == E_ARG


def test_the_file_is_built_like_the_others():
    mk = open(os.path.join(ROOT, "fcn_object_detector_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS\s*:=.*\bneuron\.hip\b", mk, flags=re.M) and "-ffp-contract=off" in mk
    src = open(os.path.join(ROOT, "fcn_object_detector_amd", "csrc", "neuron.hip")).read()
    assert "asm" not in src and "expm1f" in src and "log1pf" in src and "__shared__" not in src and "atomic" not in src.replace("no atomics", "")


def fwd(name="fcn_neuron_fwd_f32", x=X, y=Y, keep=None, p=5, c=8, xcs=16, xco=0, ycs=16, yco=0, kcs=0, mode=L.NEURON_SWISH, a=1.0, b=0.0):
    if name.endswith("f16"):
        return getattr(L.load(), name)(x, y, p, c, xcs, xco, ycs, yco, mode, a, b, None)
    return getattr(L.load(), name)(x, y, keep, p, c, xcs, xco, ycs, yco, kcs, mode, a, b, None)


def test_forward_refusals():
    err = L.load().fcn_last_error_string
    for name in NAMES[:2]:
        f16 = name.endswith("f16")
        assert fwd(name, x=None) == E_ARG and fwd(name, y=None) == E_ARG and b"null" in err()
        assert fwd(name, p=0) == E_ARG and fwd(name, c=-1) == E_ARG and b"extent" in err()
        assert fwd(name, mode=5) == E_ARG and fwd(name, mode=-1) == E_ARG and b"unknown mode" in err()
        assert fwd(name, mode=L.NEURON_ELU, a=-1e-3) == E_ARG and fwd(name, mode=L.NEURON_ELU, a=NAN) == E_ARG and b"alpha" in err()
        assert fwd(name, mode=L.NEURON_CLIP, a=2.0, b=2.0) == E_ARG and fwd(name, mode=L.NEURON_CLIP, a=2.0, b=1.0) == E_ARG
        assert fwd(name, mode=L.NEURON_CLIP, a=NAN, b=1.0) == E_ARG and b"lo < hi" in err()
        assert fwd(name, xco=16) == E_ARG and fwd(name, ycs=4) == E_ARG and fwd(name, yco=-8) == E_ARG
        assert fwd(name, xcs=20 if f16 else 18) == E_ALIGN and fwd(name, yco=4 if f16 else 2, ycs=32) == E_ALIGN
        assert fwd(name, x=X + 8) == E_ALIGN and fwd(name, y=Y + 4) == E_ALIGN
        # the parameter checks come before the views': a bad alpha on a bad view is an argument error
        assert fwd(name, mode=L.NEURON_ELU, a=-1.0, x=X + 8) == E_ARG
    assert fwd(NAMES[1], xcs=12, xco=4, c=4) == E_ALIGN      # (a window at 4 of 12 is a float32 window: halves come in groups of 8)
    assert fwd(keep=K, kcs=4) == E_ARG and fwd(keep=K, kcs=10) == E_ALIGN and fwd(keep=K + 4, kcs=8) == E_ALIGN


def test_backward_refusals():
    lib = L.load()
    bd = lambda dy=X, ref=Y, dx=K, p=5, c=8, dcs=16, dco=0, rcs=16, rco=0, xcs=16, xco=0, mode=L.NEURON_SWISH, a=1.0, b=0.0: lib.fcn_neuron_bwd_f32(
        dy, ref, dx, p, c, dcs, dco, rcs, rco, xcs, xco, mode, a, b, 0, None)
    assert bd(dy=None) == E_ARG and bd(dx=None) == E_ARG and all(bd(ref=None, mode=m) == E_ARG for m in range(5))
    assert bd(p=0) == E_ARG and bd(c=0) == E_ARG and bd(mode=9) == E_ARG and bd(xco=12) == E_ARG and bd(rco=12) == E_ARG and bd(dcs=4) == E_ARG
    assert bd(mode=L.NEURON_ELU, a=-0.5) == E_ARG and bd(mode=L.NEURON_CLIP, a=0.0, b=0.0) == E_ARG and bd(mode=L.NEURON_CLIP, a=0.0, b=NAN) == E_ARG
    assert bd(dcs=18) == E_ALIGN and bd(xco=2, xcs=32) == E_ALIGN and bd(rcs=18) == E_ALIGN and bd(dx=K + 4) == E_ALIGN and bd(ref=Y + 8) == E_ALIGN
    assert b"neuron_bwd" in lib.fcn_last_error_string()
