"""The inputs of the ArgMax tests (tests/test_argmax_ref.py asserts what is promised here; the GPU tests launch them).

Margin cases: in float64 the gap between consecutive ranks 0 .. top_k of every pixel is at least MARGIN = 2^-7 of the pixel's
largest magnitude.  A half's rounding error is 2^-11 relative, two values make 2^-10, and that leaves eight times the room: float32
and half kernels, fused or not (the unfused half-float path rounds the blend once more), must all name the same channels.  Plain
cases hold their margin by construction (the top ranks sit on a ladder of steps of 1 / 24 above the rest); fused cases - a map of
regions with one dominant class each plus noise, so that blends cross between classes as a score map's do - take the first seed at
which it holds for every output pixel.  No pixel is ever left out.

Exact-tie cases: small integers (plain, and fused at 3 x 4 -> 9 x 13, where every weight is a multiple of 1 / 4 and the blends are
exact) and constant planes (fused, any geometry: equal planes run through the same arithmetic and stay equal), with the tied maximum
at more than one channel, so that the rule - the larger index first - decides the answer."""
import functools

import numpy as np

import ref_argmax64 as R
import ref_interp64 as RI

MARGIN = 2.0 ** -7
STEP = 1.0 / 24.0


def dtype_of(half):
    return np.float16 if half else np.float32


@functools.lru_cache(maxsize=64)
def plain_margin(c, pixels, top_k, half, negative=False, seed=0):
    """(1, c, 1, pixels): ranks 0 .. min(top_k, c - 1) of every pixel are 1, 1 - STEP, 1 - 2 STEP, ... at random channels, the rest lies
    at least one STEP below the last of them.  negative: everything shifted down by 2 (an accumulator that starts at 0 would win)."""
    rng = np.random.default_rng(1000 * c + 10 * top_k + seed)
    top = min(top_k + 1, c)
    lo = 1.0 - (top - 1) * STEP
    x = rng.uniform(lo - 1.0, lo - STEP, (pixels, c))
    where = np.argsort(rng.random((pixels, c)), axis=1)[:, :top]      # `top` different channels per pixel
    np.put_along_axis(x, where, np.broadcast_to(1.0 - STEP * np.arange(top), (pixels, top)), axis=1)
    if negative:
        x -= 2.0
    return np.ascontiguousarray(x.T.reshape(1, c, 1, pixels)).astype(dtype_of(half))


def plain_ties(c, pixels, half, seed=0):
    """Small integers 0 .. 2: with more than three channels every pixel has equal values among its ranks."""
    rng = np.random.default_rng(77 + c + seed)
    return rng.integers(0, 3, (1, c, 1, pixels)).astype(dtype_of(half))


def plain_equal(c, pixels, half, value=-1.5):
    """All equal (and negative): the ranks read c - 1, c - 2, ..."""
    return np.full((1, c, 1, pixels), value, dtype_of(half))


def _regions(rng, n, c, h, w):
    label = rng.integers(0, c, (n, h, w))
    x = 0.3 * rng.standard_normal((n, c, h, w))
    np.put_along_axis(x, label[:, None], 2.0 + np.take_along_axis(x, label[:, None], axis=1), axis=1)
    return x


@functools.lru_cache(maxsize=None)
def fused_margin(n, c, h, w, oh, ow, pad_beg, pad_end, half, softmax=False):
    """(x, seed): the first seed whose blended map - and, with softmax, whose probabilities - keep MARGIN between rank 0 and rank 1 at
    every output pixel, judged on the input as the kernel reads it (rounded to the element type)."""
    for seed in range(2000):
        x = _regions(np.random.default_rng(seed), n, c, h, w).astype(dtype_of(half))
        y = RI.interp(x.astype(np.float64), oh, ow, pad_beg, pad_end)
        if R.margin(y, 1) >= MARGIN and (not softmax or R.margin(R.softmax(y), 1) >= MARGIN):
            return x, seed
    raise AssertionError("no seed below 2000 keeps the margin")


def fused_constant_planes(n, c, h, w, half):
    """Constant planes of small integers whose maximum 3 sits at channels 1 and c - 1 (and nowhere else)."""
    v = np.arange(c) % 3
    v[1], v[c - 1] = 3, 3
    return np.broadcast_to(v.reshape(1, c, 1, 1), (n, c, h, w)).astype(dtype_of(half)).copy()


def fused_integers(n, c, h, w, half, seed=0):
    """Small integers 0 .. 2 for a geometry with dyadic weights (3 x 4 -> 9 x 13): exact blends, ties at most pixels."""
    return np.random.default_rng(5 + seed).integers(0, 3, (n, c, h, w)).astype(dtype_of(half))


# the plain kernel's shapes: channels, x_cstride of the float32 / of the half view, x_coffset, pixels.  A float32 stride that is no
# multiple of 4 takes the one-element loads; halves always come in whole segments of 8.
PLAIN_SHAPES = [
    (1, 1, 8, 0, 70), (2, 2, 8, 0, 70),
    (3, 4, 8, 0, 70),            # no whole group
    (5, 16, 16, 8, 70),          # a window; pad and neighbour channels hold a huge value: reading them into the comparison would win
    (21, 24, 24, 0, 67),         # no multiple of a wave
    (31, 31, 32, 0, 70),         # the last width a lane takes at this pixel count ...
    (32, 32, 32, 0, 70),         # ... and the first that a wave takes (FCN_ARGMAX_WAVE_MIN_C channels, at most FCN_ARGMAX_WAVE_PIXELS pixels)
    (33, 33, 40, 0, 70),
    (256, 256, 256, 0, 5),
    (257, 260, 264, 0, 5),
    (1000, 1000, 1000, 0, 3),    # a classifier's rows: a wave per pixel
]
# both sides of the switch where it depends on the pixel count and on the bytes of a window (FCN_ARGMAX_WAVE_PIXELS = 8192,
# FCN_ARGMAX_WAVE_BYTES = 512): run with top_k 1 and 5 only - the ranks' logic does not change with the launch shape
SWITCH_SHAPES = [
    (32, 32, 32, 0, 8192),       # a wave per pixel ...
    (32, 32, 32, 0, 8193),       # ... a lane per pixel
    (128, 128, 128, 0, 8193),    # 512 bytes of floats: a lane
    (129, 132, 136, 0, 8193),    # 516 bytes of floats: a wave; 258 bytes of halves: a lane
    (256, 256, 256, 0, 8193),    # 512 bytes of halves: a lane
    (257, 260, 264, 0, 8193),    # 514 bytes of halves: a wave
]
# n, c, h, w, oh, ow, pad_beg, pad_end
FUSED_GEOMS = [(1, 5, 3, 4, 9, 13, 0, 0), (1, 4, 1, 1, 5, 5, 0, 0), (1, 21, 6, 7, 6, 7, 0, 0), (1, 6, 6, 7, 13, 17, -1, 0), (2, 3, 3, 4, 9, 13, 0, 0)]


def top_ks(c):
    return sorted({k for k in (1, 2, 5, c) if k <= min(c, 32)})
