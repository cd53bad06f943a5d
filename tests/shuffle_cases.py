"""The cases of tests/test_gpu_guarded_shuffle.py, shared with tests/test_shuffle_ref.py, which shows without a GPU that each of them can
fail: that it tells the permutation from its inverse (g and C / g swapped) and from the identity, and a gradient from one whose
accumulate flag was ignored.

A case is (C, g), the smallest at which each path of csrc/shuffle.hip runs:
  (6, 3), (10, 5)      a partial last group of floats (and of halves)
  (12, 3), (24, 2)     whole groups
  (72, 3), (136, 2)    more than 16 groups of floats per pixel (and, at 136, of halves): a second workgroup column
  (9, 3), (15, 5)      halves: an odd last channel, stored as one half beside a pad half of the same 32-bit word
  (12, 2), (20, 5)     halves: a last group of whole 32-bit pairs
  (16, 4)              g == C / g: the permutation is its own inverse; only the identity is told apart (so it is at (9, 3); the odd
                       last half of (15, 5) has g != C / g)
  (12, 1), (12, 12)    the identity
Every case runs in both element types.  Pixel counts per case and element type (pixel_counts): 1, and one less and one more than the
rows of a workgroup - 256 // tg, cg_tile() of csrc/chan_group.h restated in tile().  A launch has at most MAX_GROUPS = 2048
workgroups; at two workgroup columns that is 1024 of 16 pixels each along the pixels, so TRIP_F32 / TRIP_F16 - (pixels, C, g) just past
16384 pixels at 18 groups of floats / 17 of halves - take the grid-stride loop into a second trip.

Operands (operands): x[p, c] = +-(c + 1 + 137 * (p % 7)), the sign by the pixel's parity - no two channels of a pixel are equal, and
every value is an integer below 2048, exact as a half -; the gradient the bottom already holds is 0.5 * (c + 1) + 3 * (p % 5), so every
sum is exact in float32 as well."""
import numpy as np

CASES = [(6, 3), (10, 5), (12, 3), (24, 2), (72, 3), (136, 2), (9, 3), (15, 5), (12, 2), (20, 5), (16, 4), (12, 1), (12, 12)]
IDENTITY = [(12, 1), (12, 12)]
SELF_INVERSE = [(9, 3), (16, 4)]
MAX_GROUPS, THREADS = 2048, 256
TRIP_F32, TRIP_F16 = (16384 + 21, 72, 3), (16384 + 21, 136, 2)


def case_id(case) -> str:
    return "c%d_g%d" % case


def tile(pixels: int, c: int, epg: int):
    """(tg, rows, gx, gy) of a launch over `pixels` x `c` in groups of epg elements, as cg_tile(1, pixels, c, epg, 2048) computes them."""
    cg, tg = -(-c // epg), 1
    while tg < cg and tg < 16:
        tg *= 2
    rows, gx = THREADS // tg, -(-cg // tg)
    return tg, rows, gx, min(-(-pixels // rows), max(MAX_GROUPS // gx, 1))


def trips(pixels: int, c: int, epg: int) -> int:
    """Trips of the grid-stride loop taken by the workgroup that takes the most."""
    _tg, rows, _gx, gy = tile(pixels, c, epg)
    return -(-pixels // (rows * gy))


def pixel_counts(c: int, epg: int):
    rows = tile(1, c, epg)[1]
    return (1, rows - 1, rows + 1)


def operands(pixels: int, c: int, dtype=np.float32):
    """x and the pre-filled gradient y0, (1, C, 1, P), of element type dtype (y0 is used in float32 only)."""
    p, ch = np.arange(pixels)[None, :], np.arange(c)[:, None]
    x = (ch + 1 + 137 * (p % 7)) * np.where(p % 2, -1, 1)
    y0 = 0.5 * (ch + 1) + 3 * (p % 5)
    return x.astype(dtype).reshape(1, c, 1, pixels), y0.astype(dtype).reshape(1, c, 1, pixels)
