"""C ABI of the channel-shuffle kernels (csrc/shuffle.hip): symbols, prototypes against the header and lib.py, and the host-side refusals
(no GPU: every call here returns before anything touches a device)."""
import ctypes as C
import os
import re

from conftest import ROOT
from fcn_object_detector_amd import lib as L

E_ARG, E_ALIGN = 1, 2
NAMES = ("fcn_shuffle_channel_f32", "fcn_shuffle_channel_f16")
X, Y = 0x100000, 0x200000      # fake, never dereferenced, 16-byte aligned, 1 MiB apart


def header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fcnhip.h")).read(), flags=re.S)


def test_symbols_are_exported_and_bound_and_the_abi_version_stays():
    lib = L.load()
    for n in NAMES:
        assert hasattr(lib, n) and n in L.PROTOTYPES, n
    assert lib.fcn_abi_version() == 2


def test_prototypes_match_the_header():
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
    # the argument names the engines rely on, in order
    order = lambda n: [a.split()[-1].lstrip("*") for a in re.search(r"\b%s\s*\((.*?)\)" % n, txt, flags=re.S).group(1).split(",")]
    assert order(NAMES[0]) == ["x", "y", "pixels", "C", "group", "x_cstride", "x_coffset", "y_cstride", "y_coffset", "accumulate", "s"]
    assert order(NAMES[1]) == [a for a in order(NAMES[0]) if a != "accumulate"]


def test_the_file_is_built_like_the_others_on_the_channel_group_header():
    mk = open(os.path.join(ROOT, "fcn_object_detector_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS\s*:=.*\bshuffle\.hip\b", mk, flags=re.M)
    src = open(os.path.join(ROOT, "fcn_object_detector_amd", "csrc", "shuffle.hip")).read()
    assert '#include "chan_group.h"' in src and "asm" not in src and "atomic" not in src.replace("no atomics", "")
    # what the library ships: the file without its experiment block (the LDS-staged form of DESIGN.md 4.29, built only by `make exp`)
    assert src.count("#ifdef FCN_SHUFFLE_LDS") == 3 and "FCN_SHUFFLE_LDS" not in mk
    src = re.sub(r"#ifdef FCN_SHUFFLE_LDS.*?#endif\n", "", src, flags=re.S)
    assert "__shared__" not in src and "shuffle_lds" not in src
    for helper in ("cg_tile(", "cg_lane<4>", "cg_lane<8>", "cg_first(", "cg_step(", "cg_store_acc(", "cg_store_h8(", "cg_view_in(", "cg_view_ok(",
                   "cg_aligned16("):
        assert helper in src, helper
    assert "threadIdx" not in src and "blockIdx" not in src      # no lane decomposition of its own


def call(name=NAMES[0], x=X, y=Y, p=5, c=12, g=3, xcs=16, xco=0, ycs=16, yco=0, acc=0):
    fn = getattr(L.load(), name)
    return fn(x, y, p, c, g, xcs, xco, ycs, yco, None) if name.endswith("f16") else fn(x, y, p, c, g, xcs, xco, ycs, yco, acc, None)


def test_refusals():
    err = L.load().fcn_last_error_string
    for name in NAMES:
        grp = 8 if name.endswith("f16") else 4
        assert call(name, x=None) == E_ARG and call(name, y=None) == E_ARG and b"null" in err()
        assert call(name, p=0) == E_ARG and call(name, c=-1) == E_ARG and b"extent" in err()
        assert call(name, g=0) == E_ARG and call(name, g=-3) == E_ARG and call(name, g=5) == E_ARG and call(name, g=24) == E_ARG
        assert b"does not divide" in err()
        assert call(name, xco=16) == E_ARG and call(name, ycs=8) == E_ARG and call(name, yco=-grp) == E_ARG and b"out of range" in err()
        assert call(name, xcs=16 + grp // 2) == E_ALIGN and call(name, ycs=32, yco=grp // 2) == E_ALIGN and b"multiples of" in err()
        assert call(name, x=X + 8) == E_ALIGN and call(name, y=Y + 4) == E_ALIGN and b"16-byte aligned" in err()
        # x and y as windows that overlap: the same window, and y beginning inside x's bytes
        assert call(name, y=X) == E_ARG and b"overlap" in err()
        assert call(name, y=X + 16 * grp) == E_ARG and call(name, x=Y + 32, p=50) == E_ARG and b"overlap" in err()
        # the group check comes before the views': a bad group on a bad view is an argument error
        assert call(name, g=5, x=X + 8) == E_ARG
    assert call(NAMES[1], xcs=12, xco=4, c=4, g=2) == E_ALIGN      # (a window at 4 of 12 is a float32 window: halves come in groups of 8)
