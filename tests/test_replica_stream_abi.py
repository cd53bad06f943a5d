"""fcn_stream_create_replica / fcn_stream_is_prioritized without a GPU: lib.py's prototypes match include/fcnhip.h, and null pointers are
refused with FCN_E_ARG before any HIP call, whatever the index."""
import ctypes as C
import os
import re

from conftest import ROOT
from fcn_object_detector_amd import lib as L

E_ARG = 1


def _params(txt, name):
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, txt)
    assert m, name
    return [re.sub(r"\s+", "", re.sub(r"\b\w+\s*$", "", p.strip())) for p in m.group(1).split(",")]      # types, names dropped


def test_prototypes_match_the_header():
    txt = open(os.path.join(ROOT, "include", "fcnhip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    assert _params(txt, "fcn_stream_create_replica") == ["fcn_stream_t*", "int"]
    assert L.PROTOTYPES["fcn_stream_create_replica"] == (C.c_int, [C.POINTER(C.c_void_p), C.c_int])
    assert _params(txt, "fcn_stream_is_prioritized") == ["fcn_stream_t", "int*"]
    assert L.PROTOTYPES["fcn_stream_is_prioritized"] == (C.c_int, [C.c_void_p, C.POINTER(C.c_int)])
    assert "#define FCN_REPLICA_STREAMS %d\n" % L.REPLICA_STREAMS in txt


def test_null_pointers_are_refused():
    lib = L.load()
    for index in (0, 3, -1, L.REPLICA_STREAMS):
        assert lib.fcn_stream_create_replica(None, index) == E_ARG
        assert b"fcn_stream_create_replica" in lib.fcn_last_error_string()
    yes = C.c_int(7)
    assert lib.fcn_stream_is_prioritized(None, C.byref(yes)) == E_ARG and yes.value == 7
    mem = (C.c_char * 16)()
    assert lib.fcn_stream_is_prioritized(C.addressof(mem), None) == E_ARG
