"""The cases of tests/test_gpu_guarded_gate.py, shared with tests/test_gate_ref.py, which shows without a GPU that each of them can fail.

Shapes: N = 2 and 3 images; pixels per image 1, 5, 49 and 300; C = 6 (one whole 16-byte group of floats and a partial one: the scalar
path), 8 (whole groups), 20 (a partial last group behind whole ones) and 68 (more than 64 channels: two workgroups along the channels).
Slab boundary of the gate gradient, read from gate_tile() of csrc/gate.hip: a workgroup's 256 lanes stand tg = min(16, next power of
two >= ceil(C / 4)) channel groups wide and 256 / tg pixels high, and a slab is never shorter than those rows (it grows only past 2048
workgroups) - first_slab(C) pixels: 128 at C = 6 and 8, 32 at C = 20, 16 at C = 68.  So 300 pixels cross a slab boundary at every C
(3, 3, 10 and 19 slabs), 49 pixels at C = 20 and 68 (2 and 4 slabs), and 1 and 5 pixels never do.
ODD_SHAPES, for the half-float forward alone: N = 2 and the odd widths of tests/neuron_cases.py at their pixel counts, at which the store
of a partial group of halves writes a single half beside a pad half of the same 32-bit word."""
import numpy as np

import neuron_cases

# (N, H, W, C)
SHAPES = [(2, 1, 1, 6), (3, 1, 5, 8), (2, 7, 7, 20), (3, 15, 20, 68), (2, 15, 20, 6), (3, 7, 7, 68), (2, 1, 5, 20), (3, 1, 1, 8), (2, 15, 20, 20),
          (3, 7, 7, 8), (2, 15, 20, 8)]
ODD_SHAPES = [(2, 1, 5, c) if p == 5 else (2, 7, 7, c) for p, c in neuron_cases.ODD_C]


def first_slab(c: int) -> int:
    groups, tg = (c + 3) // 4, 1
    while tg < groups and tg < 16:
        tg *= 2
    return 256 // tg


def crosses_a_slab(shape) -> bool:
    n, h, w, c = shape
    return h * w > first_slab(c)


def operands(shape, seed=0):
    """x, the gate in (0.1, 0.9) and different for every image, the residual, dy and pre-filled gradients - float32, NCHW / (N, C)."""
    n, h, w, c = shape
    rng = np.random.default_rng(1000 + seed)
    x = rng.standard_normal((n, c, h, w)).astype(np.float32)
    g = (0.1 + 0.8 * rng.random((n, c))).astype(np.float32)
    r = rng.standard_normal((n, c, h, w)).astype(np.float32)
    dy = rng.standard_normal((n, c, h, w)).astype(np.float32)
    dx0 = rng.standard_normal((n, c, h, w)).astype(np.float32)
    dg0 = rng.standard_normal((n, c)).astype(np.float32)
    return x, g, r, dy, dx0, dg0
