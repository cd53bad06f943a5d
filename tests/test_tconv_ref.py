"""The float64 reference of the transposed convolution (tests/ref_tconv64.py) against three independent statements of it (no GPU)."""
import numpy as np
import pytest

import ref64
import ref_tconv64 as T
from oracle import caffe_ref

# (k, stride): the shape list of the kernel's contract
KS = [(1, 2), (2, 2), (3, 2), (4, 2), (5, 2), (7, 2), (3, 3), (16, 8), (32, 16), (2, 4), (3, 1)]


def _rng(seed):
    return np.random.default_rng(seed)


@pytest.mark.parametrize("k,s", KS)
def test_adjoint_of_the_convolution(k, s):
    """<conv(x), dy> == <x, tconv(dy)> for every input size, the ones with (H0 + 2p - k) % s != 0 included."""
    rng = _rng(k * 100 + s)
    for pad in sorted({0, k // 2, k - 1}):
        for extra in range(s):
            h0 = max(k - 2 * pad, 1) + s * 2 + extra
            w0 = h0 + 1
            if h0 + 2 * pad < k:
                continue
            x = rng.standard_normal((2, 3, h0, w0))
            w = rng.standard_normal((5, 3, k, k))
            y = ref64.conv2d(x, w, None, pad, s)
            dy = rng.standard_normal(y.shape)
            # the bank of the data gradient: a = dY has Ca = Cout channels, b = dX has Cb = Cin
            dx = T.tconv2d(dy, w, None, pad, s, (h0, w0))
            lhs, rhs = float((y * dy).sum()), float((x * dx).sum())
            assert abs(lhs - rhs) <= 1e-12 * max(abs(lhs), abs(rhs), 1.0), (k, s, pad, extra)
            if (h0 + 2 * pad - k) % s:
                unc = (h0 + 2 * pad - k) % s - pad      # rows of x under no window (when the padding does not cover them)
                if unc > 0:
                    assert np.all(dx[:, :, h0 - unc:, :] == 0.0)


@pytest.mark.parametrize("k,s", KS)
def test_equals_conv2d_dgrad(k, s):
    rng = _rng(7 + k + s)
    pad = k // 2
    for extra in range(min(s, 3)):
        h0, w0 = k + s * 2 + extra, k + s + extra
        dy = rng.standard_normal((1, 4, ref64.conv_out(h0, k, pad, s), ref64.conv_out(w0, k, pad, s)))
        w = rng.standard_normal((4, 2, k, k))
        got, want = T.tconv2d(dy, w, None, pad, s, (h0, w0)), ref64.conv2d_dgrad(dy, w, pad, s, h0, w0)
        assert np.allclose(got, want, rtol=0, atol=1e-12 * np.abs(want).max())


@pytest.mark.parametrize("k,s,pad", [(4, 2, 1), (16, 8, 4), (3, 2, 0), (2, 2, 0), (5, 2, 2), (2, 4, 1), (7, 2, 6)])
def test_equals_caffe_deconvolution_group1(k, s, pad):
    rng = _rng(k + 31 * s + pad)
    x = rng.standard_normal((2, 3, 5, 4)).astype(np.float32)
    w = rng.standard_normal((3, 6, k, k)).astype(np.float32)
    b = rng.standard_normal(6).astype(np.float32)
    want = caffe_ref.deconv2d(x, w, b, pad, s)
    got = T.tconv2d(x, w, b, pad, s)
    assert got.shape == want.shape
    assert np.abs(got - want).max() <= 1e-5 * T.tconv2d_mag(x, w, b, pad, s).max()


def test_rectangular_kernel_and_magnitude_twin():
    rng = _rng(3)
    a = rng.standard_normal((1, 2, 3, 5))
    w = rng.standard_normal((2, 3, 3, 2))
    out = T.tconv2d(a, w, None, 0, 2)
    assert out.shape == (1, 3, 2 * 2 + 3, 2 * 4 + 2)
    # brute force over the definition
    want = np.zeros_like(out)
    for oy in range(out.shape[2]):
        for ox in range(out.shape[3]):
            for r in range(3):
                for q in range(2):
                    if (oy - r) % 2 == 0 and (ox - q) % 2 == 0 and 0 <= (oy - r) // 2 < 3 and 0 <= (ox - q) // 2 < 5:
                        want[0, :, oy, ox] += a[0, :, (oy - r) // 2, (ox - q) // 2] @ w[:, :, r, q]
    assert np.allclose(out, want, rtol=0, atol=1e-13)
    assert np.all(T.tconv2d_mag(a, w, None, 0, 2) >= np.abs(out) - 1e-13)


def test_bank_layouts():
    rng = _rng(5)
    w = rng.standard_normal((5, 3, 2, 3)).astype(np.float32)
    pk, dv = T.pack_bank(w), T.device_blob(w)
    assert pk.shape == (2, 3, 3, 8) and dv.shape == (5, 2, 3, 4)
    for ca in range(5):
        for cb in range(3):
            assert np.array_equal(pk[:, :, cb, ca], w[ca, cb]) and np.array_equal(dv[ca, :, :, cb], w[ca, cb])
    assert not pk[..., 5:].any() and not dv[..., 3:].any()
    # a Convolution's OHWI bank IS the device blob of the transposed problem (Ca = Cout, Cb = Cin)
    from gpu_util import pack_ohwi
    assert np.array_equal(pack_ohwi(w), dv)


def test_output_size_outside_the_range_is_refused():
    a, w = np.zeros((1, 1, 3, 3)), np.zeros((1, 1, 3, 3))
    with pytest.raises(AssertionError):
        T.tconv2d(a, w, None, 1, 2, (7, 5))
    with pytest.raises(AssertionError):
        T.tconv2d(a, w, None, 1, 2, (4, 5))
