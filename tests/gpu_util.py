"""Helpers for the GPU parity tests: move NCHW numpy arrays to NHWC device buffers and back through the C ABI."""
import ctypes as C

import numpy as np
import pytest

from fcn_object_detector_amd import lib as L
from fcn_object_detector_amd.engine import DeviceBuffer


def dev_from(arr: np.ndarray) -> DeviceBuffer:
    a = np.ascontiguousarray(arr)
    d = DeviceBuffer(max(a.nbytes, 16), zero=False)
    L.call("fcn_memcpy_h2d_async", d.ptr, a.ctypes.data, a.nbytes, None)
    L.call("fcn_device_sync")
    return d


def dev_to(d: DeviceBuffer, shape, dtype=np.float32) -> np.ndarray:
    out = np.empty(shape, dtype)
    L.call("fcn_memcpy_d2h_async", out.ctypes.data, d.ptr, out.nbytes, None)
    L.call("fcn_device_sync")
    return out


def nhwc(x: np.ndarray, cstride=None, coffset=0, fill=0.0) -> np.ndarray:
    """NCHW -> NHWC with optional wider channel stride / offset (pad filled with `fill`)."""
    n, c, h, w = x.shape
    cs = cstride or c
    out = np.full((n, h, w, cs), fill, np.float32)
    out[..., coffset:coffset + c] = x.transpose(0, 2, 3, 1)
    return out


def nchw(y: np.ndarray, c: int, coffset=0) -> np.ndarray:
    return np.ascontiguousarray(y[..., coffset:coffset + c].transpose(0, 3, 1, 2))


def conv_desc(x_dev, w_dev, b_dev, y_dev, N, H, W, Cin, x_cstride, Cout, k, pad, stride, OH, OW, y_cstride, y_coffset=0, flags=0,
              in_shift=0.0, y2_dev=None, y2_cstride=0, y2_coffset=0):
    d = L.ConvDesc()
    d.x, d.w, d.bias, d.y = x_dev.ptr, w_dev.ptr, (b_dev.ptr if b_dev is not None else None), y_dev.ptr
    d.y2 = y2_dev.ptr if y2_dev is not None else None
    d.N, d.H, d.W, d.Cin, d.x_cstride = N, H, W, Cin, x_cstride
    d.Cout, d.kh, d.kw, d.pad, d.stride, d.OH, d.OW = Cout, k, k, pad, stride, OH, OW
    d.y_cstride, d.y_coffset, d.y2_cstride, d.y2_coffset = y_cstride, y_coffset, y2_cstride, y2_coffset
    d.flags, d.in_shift = flags, in_shift
    return d


def pack_ohwi(w: np.ndarray) -> np.ndarray:
    co, ci, kh, kw = w.shape
    ci4 = (ci + 3) // 4 * 4
    out = np.zeros((co, kh, kw, ci4), np.float32)
    out[..., :ci] = w.transpose(0, 2, 3, 1)
    return out


def adopt_device_activations(ref, eng, spec, keep=()):
    """Make the oracle's backward run on the DEVICE's forward pass: every 4-d blob of `ref` (except `keep`, the inputs) is
    replaced by the engine's, and the pooling argmaxes / LRN scales are recomputed from them.  ReLU masks and max-pool
    argmaxes are discontinuous: two independently rounded forward passes flip a handful of near-zero activations / near-tied
    windows, and a flipped mask says nothing about the backward kernels or the solver.  With identical masks what is left
    is the backward arithmetic itself, which is held to the north-star tolerance (1e-3)."""
    from oracle import caffe_ref as R
    for name in list(ref.blobs):
        if name in eng.blobs and len(eng.blobs[name].shape) == 4 and name not in keep:
            ref.blobs[name] = eng.read_blob(name).copy()
    for l in spec.layers:
        if l.type == "Pooling" and str(l.sub("pooling_param").get("pool", "MAX")) == "MAX":
            k, s_, p_ = (int(l.sub("pooling_param").get(q, d)) for q, d in (("kernel_size", 0), ("stride", 1), ("pad", 0)))
            ref.aux[l.name] = R.max_pool(ref.blobs[l.bottoms[0]], k, s_, p_, return_index=True)[1]
        elif l.type == "LRN":
            ref.aux[l.name] = R.lrn_across(ref.blobs[l.bottoms[0]], 5, 1e-4, 0.75, 1.0, return_scale=True)[1]


# ---------------------------------------------------------------------------------------------------------------------
# Guard-banded, poisoned buffers.  GPU AddressSanitizer is not available to this project, so the red zone a test lays
# down itself and reads back is the only out-of-bounds detector it has: every tensor of a guarded case lives inside one
# allocation = front red zone + payload + back red zone, everything that is not payload is filled with a poison pattern,
# and after the launch the zones must still hold the pattern bit for bit (a stray WRITE) and the result must hold no
# trace of the poison (a stray READ that was consumed).  tests/test_guard_harness.py proves each class on numpy stand-ins.
# ---------------------------------------------------------------------------------------------------------------------
POISON_WORD = 0x7FC07FC0      # float32: a quiet NaN; float16 x 2: two quiet NaNs; int32: 2143322048 (no iy*W+ix); bytes C0 7F C0 7F
HUGE_WORD_F32 = 0x7F61B1E6    # 3e38f: for MAX-pooling inputs, whose `v > m` compare ignores a NaN
HUGE_WORD_F16 = 0x7BFF7BFF    # 65504h twice
GUARD_BYTES = 256 << 10


def poison_word(poison="nan", dtype=np.float32) -> int:
    """The 32-bit pattern a region is filled with: 'nan' (POISON_WORD for every element type) or 'huge'."""
    if poison == "nan":
        return POISON_WORD
    if poison == "huge":
        return HUGE_WORD_F16 if np.dtype(dtype) == np.float16 else HUGE_WORD_F32
    return int(poison) & 0xFFFFFFFF


def poison_value(poison="nan", dtype=np.float32):
    """One element of `dtype` as the poison pattern reads there (element sizes 1, 2 and 4 tile the word)."""
    dt = np.dtype(dtype)
    return np.frombuffer(np.uint32(poison_word(poison, dt)).tobytes(), dt)[0]


def _bits(a: np.ndarray) -> np.ndarray:
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _pattern(nbytes: int, word: int) -> np.ndarray:
    """`nbytes` bytes of the repeated little-endian word, phase 0 at the allocation's first byte."""
    return np.resize(np.frombuffer(np.uint32(word).tobytes(), np.uint8), nbytes)


class GuardError(AssertionError):
    pass


class HostMemory:
    """numpy stand-in for device memory (tests/test_guard_harness.py): an allocation is a uint8 array."""

    def alloc(self, nbytes):
        a = np.zeros(nbytes, np.uint8)
        return a, a.ctypes.data

    def upload(self, handle, image):
        handle[...] = image

    def download(self, handle, offset, nbytes):
        return handle[offset:offset + nbytes].copy()

    def free(self, handle):
        pass


class DeviceMemory:
    def alloc(self, nbytes):
        d = DeviceBuffer(nbytes, zero=False)
        return d, d.ptr

    def upload(self, handle, image):
        L.call("fcn_memcpy_h2d_async", handle.ptr, image.ctypes.data, image.nbytes, None)
        L.call("fcn_device_sync")

    def download(self, handle, offset, nbytes):
        out = np.empty(nbytes, np.uint8)
        L.call("fcn_memcpy_d2h_async", out.ctypes.data, handle.ptr + offset, nbytes, None)
        L.call("fcn_device_sync")
        return out

    def free(self, handle):
        handle.free()


class GuardedBuffer:
    """One allocation = front red zone | payload | back red zone, the zones (and the up to 15 bytes that round the payload to
    16) filled with the poison pattern.  `.ptr` is the payload: 16-byte aligned, or with at_end=True placed so that its LAST
    byte is the last one before the back red zone (an over-read at the tail then reads poison at once; the start is then only
    as aligned as the payload's size).  The payload starts as `arr`, or as poison when only a size is given (an output: what a
    kernel does not write stays poison).  `.check()` reads both zones back and raises GuardError naming the first and last
    modified byte relative to the payload."""

    def __init__(self, arr_or_nbytes, guard=GUARD_BYTES, at_end=False, poison="nan", mem=None, name=""):
        arr = None if isinstance(arr_or_nbytes, (int, np.integer)) else np.ascontiguousarray(arr_or_nbytes)
        self.nbytes = int(arr_or_nbytes) if arr is None else arr.nbytes
        self.guard, self.name = int(guard), name
        assert self.guard % 16 == 0 and self.guard > 0 and self.nbytes > 0
        room = (self.nbytes + 15) // 16 * 16
        self.total = 2 * self.guard + room
        self.offset = self.guard + (room - self.nbytes if at_end else 0)
        self.word = poison_word(poison, arr.dtype if arr is not None else np.float32)
        self.mem = mem or DeviceMemory()
        self.handle, base = self.mem.alloc(self.total)
        self.ptr = base + self.offset
        self._image = _pattern(self.total, self.word)
        if arr is not None:
            self._image[self.offset:self.offset + self.nbytes] = arr.reshape(-1).view(np.uint8)
        self.mem.upload(self.handle, self._image)

    def read(self, shape, dtype=np.float32) -> np.ndarray:
        n = int(np.prod(shape)) * np.dtype(dtype).itemsize
        assert n <= self.nbytes
        return self.mem.download(self.handle, self.offset, n).view(dtype).reshape(shape)

    def modified(self):
        """(first, last) modified red-zone byte as offsets from the payload's first byte (negative: in front), or None."""
        now = self.mem.download(self.handle, 0, self.total)
        diff = now != self._image
        diff[self.offset:self.offset + self.nbytes] = False
        bad = np.nonzero(diff)[0]
        return None if bad.size == 0 else (int(bad[0]) - self.offset, int(bad[-1]) - self.offset)

    def unchanged(self) -> bool:
        """True when the WHOLE allocation - payload and both red zones - is bit-identical to what was uploaded (a refused call)."""
        return bool(np.array_equal(self.mem.download(self.handle, 0, self.total), self._image))

    def check(self):
        m = self.modified()
        if m is not None:
            first, last = m
            where = "in front of" if last < 0 else "behind" if first >= self.nbytes else "on both sides of"
            raise GuardError("red zone of %s written %s the payload (%d bytes): first modified byte at %+d, last at %+d"
                             % (self.name or "a guarded buffer", where, self.nbytes, first, last))

    def free(self):
        if self.handle is not None:
            self.mem.free(self.handle)
            self.handle = None


class Guards:
    """Every guarded buffer of one test: `with Guards() as g: xd = g.put(x); yd = g.out(y0) ...`; leaving the block checks
    every red zone (after the body's own assertions passed) and frees the allocations."""

    def __init__(self, mem=None, guard=GUARD_BYTES):
        self.mem, self.guard, self.bufs = mem, guard, []

    def put(self, arr_or_nbytes, at_end=False, poison="nan", name="") -> GuardedBuffer:
        b = GuardedBuffer(arr_or_nbytes, self.guard, at_end, poison, self.mem, name or "buffer %d" % len(self.bufs))
        self.bufs.append(b)
        return b

    def check(self):
        for b in self.bufs:
            b.check()

    def close(self):
        for b in self.bufs:
            b.free()
        self.bufs = []

    def __enter__(self):
        return self

    def __exit__(self, et, ev, tb):
        try:
            if et is None:
                self.check()
        finally:
            self.close()
        return False


def poisoned_nhwc(x: np.ndarray, cstride=None, coffset=0, poison="nan", dtype=np.float32) -> np.ndarray:
    """NCHW -> NHWC of element type `dtype`, the blob's channels at coffset .. of a pixel of cstride channels whose every
    other channel holds the poison: what a kernel sees when x is one branch of a concat buffer."""
    n, c, h, w = x.shape
    cs = cstride or c
    assert coffset >= 0 and coffset + c <= cs
    out = np.full((n, h, w, cs), poison_value(poison, dtype), dtype)
    out[..., coffset:coffset + c] = x.transpose(0, 2, 3, 1)
    return out


def poisoned(shape, poison="nan", dtype=np.float32) -> np.ndarray:
    return np.full(shape, poison_value(poison, dtype), dtype)


def slice_untouched(full: np.ndarray, coffset: int, c: int, poison="nan") -> bool:
    """True when every channel of `full` (.., cstride) outside coffset .. coffset + c - 1 still holds the poison, bit for bit
    (NaN != NaN, so the comparison goes through an integer view)."""
    keep = np.ones(full.shape[-1], bool)
    keep[coffset:coffset + c] = False
    want = _bits(np.array([poison_value(poison, full.dtype)]))[0]
    return bool(np.all(_bits(full)[..., keep] == want))


def poison_free(a: np.ndarray, poison="nan") -> bool:
    """True when no element of a result carries the poison: finite everywhere, and (for 'huge') nowhere near the huge value."""
    a = np.asarray(a)
    if a.dtype.kind != "f":
        return bool(np.all(_bits(a) != _bits(np.array([poison_value(poison, a.dtype)]))[0]))
    if not np.all(np.isfinite(a)):
        return False
    return poison != "huge" or bool(np.all(np.abs(a.astype(np.float64)) < 0.25 * float(poison_value("huge", a.dtype))))


def channels_untouched(full: np.ndarray, written: np.ndarray, poison="nan") -> bool:
    """slice_untouched for several slices of one buffer: every channel of `full` (.., cstride) whose entry in the boolean vector `written`
    is False still holds the poison, bit for bit (any element type: the comparison goes through an integer view)."""
    written = np.asarray(written, bool)
    assert written.shape == (full.shape[-1],)
    want = _bits(np.array([poison_value(poison, full.dtype)]))[0]
    return bool(np.all(_bits(full)[..., ~written] == want))


def complement(want: np.ndarray) -> np.ndarray:
    """The prefill of a BYTE output: ~want, so that a byte the kernel never wrote cannot equal its expected value (every byte value is legitimate)."""
    return np.bitwise_not(np.ascontiguousarray(want, np.uint8))


@pytest.fixture
def g(gpu):
    """The Guards of one GPU test (`from gpu_util import g`): leaving the test checks every red zone and frees the allocations."""
    with Guards() as guards:
        yield guards


def launched_twice(call, read):
    """call(); read(); call(); read() on the same buffers: both reads (an array or a sequence of arrays) must hold the same bits.  -> the first."""
    call()
    a = read()
    call()
    b = read()
    pairs = zip(a, b) if isinstance(a, (list, tuple)) else [(a, b)]
    assert all(x.tobytes() == y.tobytes() for x, y in pairs), "two launches differ"
    return a
