"""Guard-banded, bit-exact parity of the colour-augmentation kernels (csrc/augment.hip), -m gpu.

Every image lives between 256 KiB red zones; the source ends on the last byte in front of its back red zone (3 h w bytes: most of these
start at an odd address) and must be bit-identical after the launch; the destination starts as the bitwise complement of the expected
image - 0xC0 is a legitimate byte, so poison cannot show an unwritten one, a complement can; every case is launched twice on the same
buffers and must give identical bits.  Box and median blur are held to tests/ref_bytes.py (scipy.ndimage, no code shared with the kernels
or the oracle), Gauss and the colour point operations - fixed orders of float32 operations - to oracle/scene_ref.py, plus identity cases
that need no oracle.  Images 1 x 1, 2 x 9 and 7 x 5 are smaller than the kernels (the reflected border folds several times); 17 x 19 is
more than one workgroup.  All comparisons are for equality."""
import ctypes as C

import numpy as np
import pytest

import byte_cases as B
import ref_bytes as RB
from fcn_object_detector_amd import lib as L
from gpu_util import complement, g, launched_twice  # noqa: F401 (g: fixture)
from oracle import scene_ref as S

pytestmark = pytest.mark.gpu
E_ARG, E_UNSUPPORTED = 1, 3


def image_op(g, name, img, want, *args, pre=()):
    src = g.put(img, at_end=True, name="src")
    dst = g.put(complement(want), at_end=True, name="dst")
    got = launched_twice(lambda: L.call(name, src.ptr, dst.ptr, *pre, img.shape[0], img.shape[1], *args, None), lambda: dst.read(img.shape, np.uint8))
    assert src.unchanged(), "the source image was written"
    assert got.tobytes() == want.tobytes(), "%s: %d bytes differ" % (name, int((got != want).sum()))


def colour_params(fields):
    centre, off, add, mul, ga, keep = fields
    return L.ColorParams(centre, off, (C.c_int32 * 3)(*add), (C.c_float * 3)(*mul), ga, keep)


@pytest.mark.parametrize("k", B.BOX_KS)
@pytest.mark.parametrize("hw", B.IMAGE_SIZES, ids=str)
def test_box_blur(g, hw, k):
    img = B.image(hw)
    image_op(g, "fcn_blur_box_bgr8", img, RB.blur_box(img, k), k)


@pytest.mark.parametrize("k", B.MEDIAN_KS)
@pytest.mark.parametrize("hw", B.IMAGE_SIZES, ids=str)
def test_median_blur(g, hw, k):
    img = B.image(hw)
    image_op(g, "fcn_blur_median_bgr8", img, RB.blur_median(img, k), k)


@pytest.mark.parametrize("taps", list(B.GAUSS))
@pytest.mark.parametrize("hw", B.IMAGE_SIZES, ids=str)
def test_gauss_blur(g, hw, taps):
    """tmp is exactly h * w * 3 floats of NaN poison: the vertical pass must read only what the horizontal pass wrote."""
    img, t = B.image(hw), B.GAUSS[taps]
    want = img if taps == "radius0" else S.blur_gauss(img, t)
    tmp = g.put(img.size * 4, name="tmp")
    image_op(g, "fcn_blur_gauss_bgr8", img, want, t.ctypes.data, len(t) - 1, pre=(tmp.ptr,))
    assert np.all(np.isfinite(tmp.read((img.size,)))), "an element of tmp was not written"


@pytest.mark.parametrize("case", list(B.COLOUR) + ["identity"])
@pytest.mark.parametrize("hw", B.IMAGE_SIZES, ids=str)
def test_colour_point_operations(g, hw, case):
    img = B.image(hw)
    if case == "identity":
        q, want = colour_params(B.COLOUR_IDENTITY), img
    else:
        q, want = colour_params(B.colour_fields(B.COLOUR[case])), B.colour_expected(img, B.COLOUR[case])
    image_op(g, "fcn_color_augment_bgr8", img, want, C.byref(q))


def test_refusals_leave_the_buffers_alone(g):
    img = B.image((7, 5))
    h, w = img.shape[:2]
    src, dst = g.put(img, at_end=True, name="src"), g.put(complement(img), at_end=True, name="dst")
    tmp = g.put(img.size * 4, name="tmp")
    taps = B.GAUSS["sigma0.7"]
    long_taps = np.zeros(17, np.float32)
    q = colour_params(B.COLOUR_IDENTITY)
    lib = L.load()
    refused = [
        lib.fcn_blur_box_bgr8(None, dst.ptr, h, w, 3, None), lib.fcn_blur_box_bgr8(src.ptr, None, h, w, 3, None),            # null
        lib.fcn_blur_box_bgr8(src.ptr, src.ptr, h, w, 3, None),                                                              # src == dst
        lib.fcn_blur_box_bgr8(src.ptr, dst.ptr, 0, w, 3, None), lib.fcn_blur_box_bgr8(src.ptr, dst.ptr, h, -1, 3, None),     # extents
        lib.fcn_blur_box_bgr8(src.ptr, dst.ptr, 1 << 14, 1 << 14, 3, None),
        lib.fcn_blur_box_bgr8(src.ptr, dst.ptr, h, w, 0, None), lib.fcn_blur_box_bgr8(src.ptr, dst.ptr, h, w, 16, None),     # unsupported k
        lib.fcn_blur_median_bgr8(None, dst.ptr, h, w, 3, None), lib.fcn_blur_median_bgr8(src.ptr, src.ptr, h, w, 3, None),
        lib.fcn_blur_median_bgr8(src.ptr, dst.ptr, h, 0, 3, None),
        lib.fcn_blur_gauss_bgr8(src.ptr, dst.ptr, None, h, w, taps.ctypes.data, len(taps) - 1, None),
        lib.fcn_blur_gauss_bgr8(src.ptr, dst.ptr, tmp.ptr, h, w, None, 3, None),
        lib.fcn_blur_gauss_bgr8(src.ptr, src.ptr, tmp.ptr, h, w, taps.ctypes.data, len(taps) - 1, None),
        lib.fcn_blur_gauss_bgr8(src.ptr, dst.ptr, tmp.ptr, h, w, long_taps.ctypes.data, 16, None),
        lib.fcn_blur_gauss_bgr8(src.ptr, dst.ptr, tmp.ptr, h, w, taps.ctypes.data, -1, None),
        lib.fcn_blur_gauss_bgr8(src.ptr, dst.ptr, tmp.ptr, 0, w, taps.ctypes.data, len(taps) - 1, None),
        lib.fcn_color_augment_bgr8(src.ptr, dst.ptr, h, w, None, None), lib.fcn_color_augment_bgr8(src.ptr, src.ptr, h, w, C.byref(q), None),
        lib.fcn_color_augment_bgr8(None, dst.ptr, h, w, C.byref(q), None), lib.fcn_color_augment_bgr8(src.ptr, dst.ptr, 0, 0, C.byref(q), None),
    ]
    assert all(rc == E_ARG for rc in refused), refused
    for k in (1, 2, 4, 6, 9):
        assert lib.fcn_blur_median_bgr8(src.ptr, dst.ptr, h, w, k, None) == E_UNSUPPORTED, k
    L.call("fcn_device_sync")
    assert src.unchanged() and dst.unchanged() and tmp.unchanged()
