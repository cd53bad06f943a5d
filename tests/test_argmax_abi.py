"""C ABI of the ArgMax kernels: symbols, prototypes against the header, flag values, host-side refusals (no GPU: every call here
returns before anything touches a device)."""
import ctypes as C
import os
import re

import pytest

from conftest import ROOT
from fcn_object_detector_amd import lib as L

E_ARG, E_ALIGN, E_UNSUPPORTED = 1, 2, 3
PLAIN = ("fcn_argmax_fwd_f32", "fcn_argmax_fwd_f16")
FUSED = ("fcn_interp_argmax_fwd_f32", "fcn_interp_argmax_fwd_f16")
X, Y = 0x100000, 0x200000      # fake, never dereferenced, 16-byte aligned


def header():
    return open(os.path.join(ROOT, "include", "fcnhip.h")).read()


def test_symbols_are_exported_and_bound():
    lib = L.load()
    for n in PLAIN + FUSED:
        assert hasattr(lib, n) and n in L.PROTOTYPES, n
    assert lib.fcn_abi_version() == 2


def test_prototypes_match_the_header():
    txt = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    kinds = {"int": C.c_int, "fcn_stream_t": C.c_void_p}
    for n in PLAIN + FUSED:
        m = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % n, txt, flags=re.S)
        assert m, n
        want = []
        for arg in m.group(1).split(","):
            arg = " ".join(arg.split())
            want.append(C.c_void_p if "*" in arg else kinds[arg.rsplit(" ", 1)[0].replace("const ", "")])
        res, args = L.PROTOTYPES[n]
        assert res is C.c_int and list(args) == want, n


def test_flag_values_and_limits():
    defs = dict(re.findall(r"#define\s+(FCN_ARGMAX_\w+)\s+(\d+)", header()))
    assert defs == {"FCN_ARGMAX_MAX_TOPK": "32", "FCN_ARGMAX_WAVE_BYTES": "512", "FCN_ARGMAX_WAVE_PIXELS": "8192", "FCN_ARGMAX_WAVE_MIN_C": "32",
                    "FCN_ARGMAX_VALUES": "1", "FCN_ARGMAX_PAIRS": "2", "FCN_ARGMAX_SOFTMAX": "4"}
    assert (L.ARGMAX_MAX_TOPK, L.ARGMAX_VALUES, L.ARGMAX_PAIRS, L.ARGMAX_SOFTMAX) == (32, 1, 2, 4)
    assert (L.ARGMAX_WAVE_BYTES, L.ARGMAX_WAVE_PIXELS, L.ARGMAX_WAVE_MIN_C) == (512, 8192, 32)
    assert re.search(r"#define FCN_ABI_VERSION 2\b", header())


def plain(name, x=X, y=Y, pixels=7, C_=40, xcs=40, xco=0, k=1, ycs=4, yco=0, flags=0):
    return getattr(L.load(), name)(x, y, pixels, C_, xcs, xco, k, ycs, yco, flags, None)


def fused(name, x=X, y=Y, N=2, H=9, W=11, C_=5, xcs=8, xco=0, pb=-1, pe=-2, OH=12, OW=7, ycs=4, yco=0, flags=0):
    return getattr(L.load(), name)(x, y, N, H, W, C_, xcs, xco, pb, pe, OH, OW, ycs, yco, flags, None)


@pytest.mark.parametrize("name", PLAIN)
def test_plain_refusals(name):
    for bad in (dict(x=None), dict(y=None), dict(pixels=0), dict(C_=0), dict(k=0), dict(k=41), dict(k=-1),
                dict(xco=8), dict(xco=-8), dict(yco=4), dict(yco=-4), dict(k=3, flags=L.ARGMAX_PAIRS),      # 6 floats in a pixel of 4
                dict(flags=8), dict(flags=-1), dict(flags=L.ARGMAX_VALUES | L.ARGMAX_PAIRS)):
        assert plain(name, **bad) == E_ARG, bad
        assert L.load().fcn_last_error_string().decode().startswith("argmax_fwd")
    assert plain(name, k=33, ycs=36) == E_UNSUPPORTED
    assert plain(name, C_=20, k=21) == E_ARG      # above C first, whatever the limit


def test_alignment_rules_by_element_type():
    for bad in (dict(xcs=44), dict(xcs=48, xco=4), dict(ycs=6), dict(ycs=8, yco=2), dict(x=X + 8), dict(y=Y + 8)):
        assert plain("fcn_argmax_fwd_f16", **bad) == E_ALIGN, bad
    for bad in (dict(xcs=12), dict(xcs=16, xco=4), dict(ycs=6), dict(ycs=8, yco=2), dict(x=X + 8), dict(y=Y + 4)):
        assert fused("fcn_interp_argmax_fwd_f16", **bad) == E_ALIGN, bad
    # float32 has one-element loads for views that are no whole segments: only the element's own alignment is asked
    assert plain("fcn_argmax_fwd_f32", x=X + 2) == E_ALIGN and plain("fcn_argmax_fwd_f32", y=Y + 1) == E_ALIGN
    assert fused("fcn_interp_argmax_fwd_f32", x=X + 2) == E_ALIGN and fused("fcn_interp_argmax_fwd_f32", y=Y + 3) == E_ALIGN


@pytest.mark.parametrize("name", FUSED)
def test_fused_refusals(name):
    for bad in (dict(x=None), dict(y=None), dict(N=0), dict(H=0), dict(W=0), dict(C_=0), dict(OH=0), dict(OW=0),
                dict(pb=1), dict(pe=1), dict(pb=-4, pe=-5), dict(xco=4), dict(xco=-8), dict(yco=4), dict(yco=-4),
                dict(yco=3, ycs=4, flags=L.ARGMAX_PAIRS),                                       # two floats from channel 3 of 4
                dict(flags=8), dict(flags=L.ARGMAX_VALUES | L.ARGMAX_PAIRS)):
        assert fused(name, **bad) == E_ARG, bad
        assert L.load().fcn_last_error_string().decode().startswith("interp_argmax_fwd")
    assert fused(name, OW=(1 << 24) + 1) == E_UNSUPPORTED
    assert fused(name, N=1 << 10, OH=1 << 11, OW=1 << 11, H=4, W=4, pb=0, pe=0) == E_UNSUPPORTED      # 2^32 output pixels
