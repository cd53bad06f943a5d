"""The cases of tests/test_gpu_guarded_act.py, shared with tests/test_act_ref.py, which shows without a GPU that each of them can fail.

A case is (pixels, C).  C = 6 (one whole 16-byte group of floats and a partial one), 8 (whole groups), 10 (a partial group in both
element types), 20 (a partial last group behind whole ones) and 68 (more than 64 channels: two workgroups along the channels).
Pixels: 1, 5, 49 and 300, then the slab boundary of the parameter gradient, read from act_tile() of csrc/act.hip (batchnorm.hip's
formula): a workgroup's 256 lanes stand tg = min(16, next power of two >= ceil(C / 4)) channel groups wide and 256 / tg pixels high, and
a slab is never shorter than those rows (it grows only past 2048 workgroups) - first_slab(C) pixels: 128 at C = 6 and 8, 64 at C = 10,
32 at C = 20, 16 at C = 68.  One count on each side of that boundary at every C but 8 (128 | 129, 64 | 65, 32 | 33, 16 | 17), and two
counts that give more than 64 slabs - the second launch strides the slabs by 64, so slab 64 is the first that a lane adds to one it
already holds: 1041 pixels at C = 68 (66 slabs) and 4161 at C = 10 (66 slabs).
ODD_C, for the half-float forward alone: the odd widths of tests/neuron_cases.py at their pixel counts, at which the store of a partial
group of halves writes a single half beside a pad half of the same 32-bit word.

Operands: x carries EXACT zeros (every fourth element or so: where `x > 0` and `x >= 0` part ways) ; the slopes have both signs and a
zero, the shared slope is negative (a negative slope makes sign(y) differ from sign(x): a data gradient that looked at y instead of
the kept x is then wrong); dy and the pre-filled gradients are standard normal."""
import numpy as np

import neuron_cases

CASES = [(1, 6), (5, 8), (49, 10), (300, 20), (300, 68), (49, 68), (5, 20), (1, 10), (300, 6), (49, 8), (300, 10),
         (128, 6), (129, 6), (64, 10), (65, 10), (32, 20), (33, 20), (16, 68), (17, 68), (1041, 68), (4161, 10)]
ODD_C = list(neuron_cases.ODD_C)
SHARED_SLOPE = -0.35


def case_id(case) -> str:
    return "p%d_c%d" % case


def first_slab(c: int) -> int:
    groups, tg = (c + 3) // 4, 1
    while tg < groups and tg < 16:
        tg *= 2
    return 256 // tg


def slabs(case) -> int:
    p, c = case
    return -(-p // first_slab(c))


def crosses_a_slab(case) -> bool:
    return slabs(case) > 1


def workspace_bytes(case) -> int:
    """fcn_act_workspace_bytes: the slabs' sums, then one more row for the per-channel sums of a shared parameter; round4(C) floats each."""
    p, c = case
    return (slabs(case) + 1) * ((c + 3) // 4 * 4) * 4


def operands(case, seed=0):
    """x (1, C, 1, P) with exact zeros, slopes (C,) of both signs and a zero, the bias (C,), dy and a pre-filled dx - float32."""
    p, c = case
    rng = np.random.default_rng(2000 + seed + 7 * p + c)
    x = rng.standard_normal((1, c, 1, p)).astype(np.float32)
    x[rng.random(x.shape) < 0.25] = 0.0
    x.reshape(-1)[0] = 0.0                      # (a single pixel too has its zero ...
    x.reshape(-1)[-1] = -1.5                    # ... and its negative input)
    a = rng.uniform(-0.6, 0.6, c).astype(np.float32)
    a[0], a[1], a[2], a[c - 1] = 0.0, -0.45, 0.3, -0.25
    b = rng.standard_normal(c).astype(np.float32)
    dy = rng.standard_normal((1, c, 1, p)).astype(np.float32)
    dx0 = rng.standard_normal((1, c, 1, p)).astype(np.float32)
    return x, a, b, dy, dx0
