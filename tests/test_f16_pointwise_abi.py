"""Argument validation of the five half-float pointwise entry points (no GPU needed): every check precedes the first HIP call, so fake
non-null 16-byte-aligned addresses are enough - nothing is ever launched here."""
import pytest

from fcn_object_detector_amd import lib as L

E_ARG, E_ALIGN = 1, 2
A, B, Y = 0x10000, 0x20000, 0x30000      # "device" addresses: non-null, 16-byte aligned, never dereferenced


@pytest.fixture(scope="module")
def lib():
    return L.load()


def err(lib):
    return lib.fcn_last_error_string().decode()


def avepool(lib, x=A, y=Y, n=1, h=8, w=8, c=11, xcs=16, k=2, s=2, p=0, oh=4, ow=4, ycs=16, yo=0):
    return lib.fcn_avepool_fwd_f16(x, y, n, h, w, c, xcs, k, s, p, oh, ow, ycs, yo, None)


def deconv(lib, x=A, w=B, y=Y, n=1, h=3, wd=2, c=11, xcs=16, k=4, s=2, p=1, oh=6, ow=4, ycs=16, yo=0, out_f32=0):
    return lib.fcn_deconv_depthwise_fwd_f16(x, w, None, y, n, h, wd, c, xcs, k, s, p, oh, ow, ycs, yo, out_f32, None)


def eltwise(lib, a=A, b=B, y=Y, count=64, op=L.ELT_SUM):
    return lib.fcn_eltwise_fwd_f16(a, b, y, count, op, 1.0, 1.0, None)


def softmax(lib, x=A, y=Y, pixels=4, c=11, xcs=16, ycs=16, out_f32=0):
    return lib.fcn_softmax_fwd_f16(x, y, pixels, c, xcs, ycs, out_f32, None)


def copy(lib, src=A, dst=Y, pixels=4, c=11, scs=16, sco=0, dcs=32, dco=8):
    return lib.fcn_copy_channels_f16(src, dst, pixels, c, scs, sco, dcs, dco, None)


CALLS = {"avepool_f16": avepool, "deconv_depthwise_f16": deconv, "eltwise_f16": eltwise, "softmax_f16": softmax, "copy_channels_f16": copy}


@pytest.mark.parametrize("name,bad", [
    ("avepool_f16", dict(x=None)), ("avepool_f16", dict(y=None)), ("avepool_f16", dict(n=0)), ("avepool_f16", dict(c=0)), ("avepool_f16", dict(oh=0)),
    ("avepool_f16", dict(k=0)), ("avepool_f16", dict(c=17)), ("avepool_f16", dict(yo=8)),
    ("deconv_depthwise_f16", dict(x=None)), ("deconv_depthwise_f16", dict(w=None)), ("deconv_depthwise_f16", dict(y=None)),
    ("deconv_depthwise_f16", dict(h=0)), ("deconv_depthwise_f16", dict(c=0)), ("deconv_depthwise_f16", dict(oh=7)), ("deconv_depthwise_f16", dict(c=17)),
    ("eltwise_f16", dict(a=None)), ("eltwise_f16", dict(b=None)), ("eltwise_f16", dict(y=None)), ("eltwise_f16", dict(count=0)), ("eltwise_f16", dict(op=7)),
    ("softmax_f16", dict(x=None)), ("softmax_f16", dict(y=None)), ("softmax_f16", dict(pixels=0)), ("softmax_f16", dict(c=0)), ("softmax_f16", dict(c=17)),
    ("copy_channels_f16", dict(src=None)), ("copy_channels_f16", dict(dst=None)), ("copy_channels_f16", dict(pixels=0)), ("copy_channels_f16", dict(c=0)),
    ("copy_channels_f16", dict(sco=8)),
])
def test_null_pointers_and_empty_extents_are_argument_errors(lib, name, bad):
    assert CALLS[name](lib, **bad) == E_ARG
    assert name in err(lib)


@pytest.mark.parametrize("name,bad", [
    ("avepool_f16", dict(xcs=20)), ("avepool_f16", dict(ycs=20)), ("avepool_f16", dict(ycs=24, yo=4)), ("avepool_f16", dict(x=A + 8)), ("avepool_f16", dict(y=Y + 2)),
    ("deconv_depthwise_f16", dict(xcs=12)), ("deconv_depthwise_f16", dict(ycs=20)), ("deconv_depthwise_f16", dict(ycs=24, yo=4)),
    ("deconv_depthwise_f16", dict(ycs=14, out_f32=1)), ("deconv_depthwise_f16", dict(ycs=16, yo=2, out_f32=1)), ("deconv_depthwise_f16", dict(y=Y + 4)),
    ("eltwise_f16", dict(count=60)), ("eltwise_f16", dict(a=A + 2)), ("eltwise_f16", dict(y=Y + 8)),
    ("softmax_f16", dict(xcs=12)), ("softmax_f16", dict(ycs=20)), ("softmax_f16", dict(ycs=14, out_f32=1)), ("softmax_f16", dict(x=A + 8)),
    ("copy_channels_f16", dict(scs=12)), ("copy_channels_f16", dict(dcs=36)), ("copy_channels_f16", dict(dst=Y + 2)),
])
def test_strides_offsets_and_pointers_off_a_16_byte_segment_are_alignment_errors(lib, name, bad):
    assert CALLS[name](lib, **bad) == E_ALIGN
    assert name in err(lib)


def test_half_outputs_count_their_strides_in_halves(lib):
    """12 floats per pixel (11 channels) are whole 16-byte segments, 12 halves are not: the out_f32 = 0 forms refuse the stride."""
    assert deconv(lib, ycs=12, c=11, out_f32=0) == E_ALIGN and softmax(lib, ycs=12, c=11, out_f32=0) == E_ALIGN
