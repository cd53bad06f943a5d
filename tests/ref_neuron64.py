"""Float64 forward and data gradient of the five modes of csrc/neuron.hip, written from the layers' definitions (plain numpy; it imports
nothing of the package, so the mode names here are its own).  a = alpha (ELU), beta (Swish) or lo (Clip); b = hi (Clip).

  ELU     y = x > 0 ? x : a * expm1(x)                       dx = dy * (y > 0 ? 1 : y + a)             reads y
  CLIP    y = min(max(x, a), b)   (ReLU6: a = 0, b = 6)      dx = dy * [a < y < b]                      reads y
  ABSVAL  y = |x|                                            dx = dy * sign(x), sign(0) = 0             reads x
  BNLL    y = x > 0 ? x + log1p(exp(-x)) : log1p(exp(x))     dx = dy * (-expm1(-y))                     reads y
  SWISH   y = x * s, s = 1 / (1 + exp(-a x))                 dx = dy * (a y + s (1 - a y))              reads x

bwd takes `ref`, the blob the gradient reads: the layer's OUTPUT for ELU, CLIP and BNLL, its INPUT for ABSVAL and SWISH (READS says
which).  Blobs have any shape; dx_old, where given, is added (the accumulating launch)."""
import numpy as np

ELU, CLIP, ABSVAL, BNLL, SWISH = "elu", "clip", "absval", "bnll", "swish"
MODES = (ELU, CLIP, ABSVAL, BNLL, SWISH)
READS = {ELU: "y", CLIP: "y", ABSVAL: "x", BNLL: "y", SWISH: "x"}


def f64(a):
    return np.asarray(a, np.float64)


def _sigmoid(z):
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(-z))


def fwd(mode, x, a=0.0, b=0.0):
    x, a, b = f64(x), float(a), float(b)
    with np.errstate(over="ignore"):
        if mode == ELU:
            return np.where(x > 0, x, a * np.expm1(np.minimum(x, 0.0)))
        if mode == CLIP:
            return np.minimum(np.maximum(x, a), b)
        if mode == ABSVAL:
            return np.abs(x)
        if mode == BNLL:
            return np.where(x > 0, x + np.log1p(np.exp(-np.abs(x))), np.log1p(np.exp(-np.abs(x))))
        if mode == SWISH:
            return x * _sigmoid(a * x)
    raise ValueError(mode)


def bwd(mode, dy, ref, a=0.0, b=0.0, dx_old=None):
    dy, r, a, b = f64(dy), f64(ref), float(a), float(b)
    if mode == ELU:
        dx = dy * np.where(r > 0, 1.0, r + a)
    elif mode == CLIP:
        dx = dy * ((r > a) & (r < b))
    elif mode == ABSVAL:
        dx = dy * np.sign(r)
    elif mode == BNLL:
        dx = dy * -np.expm1(-r)
    elif mode == SWISH:
        s = _sigmoid(a * r)
        ay = a * r * s
        dx = dy * (ay + s * (1.0 - ay))
    else:
        raise ValueError(mode)
    return dx if dx_old is None else dx + f64(dx_old)


def ref_of(mode, x, a=0.0, b=0.0):
    """The blob bwd reads for this mode: fwd(x) or x itself."""
    return fwd(mode, x, a, b) if READS[mode] == "y" else f64(x)


def rel_err(a, b):
    """The project's measure: max |a - b| over max |b|."""
    b = f64(b)
    return float(np.abs(f64(a) - b).max() / max(np.abs(b).max(), 1e-30))
