"""Guard-banded test of work on replica streams (run with -m gpu): kernels enqueued on four streams from fcn_stream_create_replica at
once, each on an odd-sized slice between bands of a poison pattern, write their slice and nothing else.  (tests/test_guard_coverage.py
wants every entry point of include/fcnhip.h called from a guarded file or listed in its own hand-written sets, and lets a guarded file
name no stream plumbing: hence this file, and the two calls in tests/replica_stream_util.py.)"""
import ctypes as C

import numpy as np
import pytest

from replica_stream_util import finish, give_back
from fcn_object_detector_amd import lib as L
from fcn_object_detector_amd.engine import DeviceBuffer

pytestmark = pytest.mark.gpu
BAND = 64                      # floats of poison on either side of every live region
POISON = np.uint32(0x7FC0DEAD)


@pytest.mark.parametrize("n", [1003, 70001])
def test_kernels_on_replica_streams_write_only_their_slices(gpu, n):
    lib = L.load()
    rng = np.random.default_rng(n)
    streams, bufs = [], []
    for index in range(4):
        s = C.c_void_p()
        L.call("fcn_stream_create_replica", C.byref(s), index)
        yes = C.c_int(0)
        L.call("fcn_stream_is_prioritized", s, C.byref(yes))
        assert yes.value == 1, index
        streams.append(int(s.value))
    for k in range(4):
        x = rng.standard_normal(n).astype(np.float32)
        img = np.full(2 * (n + 2 * BAND), POISON, np.uint32)      # [band | x | band] [band | y | band]
        img[BAND:BAND + n] = x.view(np.uint32)
        d = DeviceBuffer(img.nbytes, zero=False)
        L.call("fcn_memcpy_h2d_async", d.ptr, img.ctypes.data, img.nbytes, None)
        bufs.append((d, x, img))
    L.call("fcn_device_sync")
    for st, (d, x, img) in zip(streams, bufs):      # all four enqueued before any is waited for
        L.check(lib.fcn_relu_fwd_f32(d.ptr + 4 * BAND, d.ptr + 4 * (n + 3 * BAND), n, 0.0, st))
    for st in streams:
        finish(st)
    for k, (d, x, img) in enumerate(bufs):
        got = np.empty_like(img)
        L.call("fcn_memcpy_d2h_async", got.ctypes.data, d.ptr, got.nbytes, None)
        L.call("fcn_device_sync")
        y0 = n + 3 * BAND
        assert np.array_equal(got[y0:y0 + n].view(np.float32), np.maximum(x, 0)), k
        assert np.array_equal(got[:y0], img[:y0]) and np.array_equal(got[y0 + n:], img[y0 + n:]), k      # x and every band untouched
    for st in streams:
        give_back(st)
    for d, _, _ in bufs:
        d.free()
