"""The cases of tests/test_gpu_guarded_neuron.py, shared with tests/test_neuron_ref.py, which shows without a GPU that each of them can fail.

A case is (pixels, C): {1, 5, 49, 300} x {6, 8, 10, 20, 68}.  C = 6 (one whole 16-byte group of floats and a partial one; a partial
group of halves), 8 (whole groups), 10 and 20 (a partial last group in both element types), 68 (17 groups of floats per pixel: the 16
lanes of a row wrap, so the second workgroup along the channels owns one group; 9 groups of halves).  ODD_C adds the widths at which the
half kernel stores a single half beside a pad half of the same 32-bit word.

A configuration is (name, mode, a, b), the mode by its name in tests/ref_neuron64.py: ELU with alpha 1, 0 and 0.7; Clip as ReLU6 (0, 6)
and with two negative bounds; AbsVal; BNLL; Swish with beta 1, a negative beta and beta 0 (y = x / 2).

Operands: one x per case, for every configuration.  Every twelfth element, in turn, is exactly 0, 6, -3.5, -0.5 (the bounds of both
Clip configurations and the kink of the other modes), 25 and -22 (beyond +-20: where exp saturates, where expm1(x) is -1 to the last
bit and BNLL is x itself); the others are 3 * standard normal.  All six special values are halves, so they stay exact in both element
types, and a single pixel of 6 channels holds each of them once.  dy and the pre-filled gradient are standard normal.

More than one trip of the grid-stride loop: neuron_tile() of csrc/neuron.hip restated (tile()).  A launch has at most MAX_GROUPS = 2048
workgroups; along the pixels that is 2048 // gx of 256 // tg pixels each.  At C = 68 floats (tg 16, gx 2) the loop takes a second trip
past 16384 pixels, at C = 68 halves (tg 16, gx 1) past 32768: TRIP_F32 and TRIP_F16, a few MB each, run once per entry point."""
import itertools

import numpy as np

import ref_neuron64 as R

PIXELS, WIDTHS = (1, 5, 49, 300), (6, 8, 10, 20, 68)
CASES = list(itertools.product(PIXELS, WIDTHS))
ODD_C = [(5, 5), (49, 13), (5, 7), (49, 3)]       # halves: 2 pairs + 1, whole group + 2 pairs + 1, 3 pairs + 1, 1 pair + 1
CONFIGS = [("elu", R.ELU, 1.0, 0.0), ("elu alpha 0", R.ELU, 0.0, 0.0), ("elu alpha 0.7", R.ELU, 0.7, 0.0),
           ("relu6", R.CLIP, 0.0, 6.0), ("clip -3.5 -0.5", R.CLIP, -3.5, -0.5), ("absval", R.ABSVAL, 0.0, 0.0), ("bnll", R.BNLL, 0.0, 0.0),
           ("swish", R.SWISH, 1.0, 0.0), ("swish beta -1.3", R.SWISH, -1.3, 0.0), ("swish beta 0", R.SWISH, 0.0, 0.0)]
SPECIAL = (0.0, 6.0, -3.5, -0.5, 25.0, -22.0)
MAX_GROUPS, THREADS = 2048, 256
TRIP_F32, TRIP_F16 = (16384 + 21, 68), (32768 + 21, 68)


def case_id(case) -> str:
    return "p%d_c%d" % case


def tile(pixels: int, c: int, epg: int):
    """(tg, rows, gx, gy) of a launch over `pixels` x `c` in groups of epg elements, as neuron_tile() computes them."""
    cg, tg = -(-c // epg), 1
    while tg < cg and tg < 16:
        tg *= 2
    rows, gx = THREADS // tg, -(-cg // tg)
    return tg, rows, gx, min(-(-pixels // rows), max(MAX_GROUPS // gx, 1))


def trips(pixels: int, c: int, epg: int) -> int:
    """Trips of the grid-stride loop taken by the workgroup that takes the most."""
    _tg, rows, _gx, gy = tile(pixels, c, epg)
    return -(-pixels // (rows * gy))


def operands(case, seed=0):
    """x (1, C, 1, P) with the special values, dy and a pre-filled dx - float32."""
    p, c = case
    rng = np.random.default_rng(4000 + seed + 7 * p + c)
    x = (3.0 * rng.standard_normal((1, c, 1, p))).astype(np.float32)
    flat = x.reshape(-1)
    for k, v in enumerate(SPECIAL):
        flat[k::12] = v
    dy = rng.standard_normal((1, c, 1, p)).astype(np.float32)
    dx0 = rng.standard_normal((1, c, 1, p)).astype(np.float32)
    return x, dy, dx0
