"""Inputs of the region-stage cases that tests/test_gpu_guarded_region.py runs on the GPU, generated here so that the no-GPU margin check
(tests/test_region_ref.py) sees exactly the same arrays: a case whose float64 decisions are closer than MARGIN to a threshold or to a
breakpoint fails there, on the CPU, before any GPU time is spent.  The seeds were chosen so that every case holds the margin."""
import functools

import numpy as np

import ref_region64 as R

MARGIN = 1e-4       # the SSD tests' figure: two orders above the float32 rounding of a score, an overlap or a bin edge

SMALL = dict(ratios=(0.5, 1.0, 2.0), scales=(1.0, 2.0, 4.0))      # 16 .. 64 pixel anchors for the small maps
# name -> parameters.  The image is (H, W) * feat_stride; shrink: mean of dw / dh (negative: boxes smaller than their anchors);
# jitter: the deltas' spread (small: neighbouring anchors decode to boxes that overlap); ties: plant equal scores among the best
PROPOSALS = {
    "m5x7":         dict(H=5, W=7, pre=100, post=20, nms=0.7, min_size=16, shrink=0.3, jitter=0.05, seed=1, **SMALL),
    "m12x10_tiles": dict(H=12, W=10, pre=150, post=60, nms=0.5, min_size=24, shrink=0.2, jitter=0.05, seed=2, ties=True, **SMALL),
    "filter_clip":  dict(H=5, W=7, pre=100, post=30, nms=0.7, min_size=24, shrink=-0.7, shift=1.5, seed=3, **SMALL),
    "few_survive":  dict(H=3, W=4, pre=100, post=40, nms=0.3, min_size=16, shrink=0.3, seed=4, **SMALL),
    "post_cut":     dict(H=5, W=7, pre=100, post=5, nms=0.7, min_size=16, shrink=-0.3, seed=5, **SMALL),
    "pre_above":    dict(H=5, W=7, pre=6000, post=50, nms=0.5, min_size=16, shrink=0.0, seed=6, **SMALL),
    "rfcn_full":    dict(H=38, W=63, pre=6000, post=300, nms=0.7, min_size=16, shrink=-0.5, jitter=0.1, seed=7, ratios=(0.5, 1.0, 2.0),
                         scales=(8.0, 16.0, 32.0)),
}
FEAT_STRIDE = 16


@functools.lru_cache(maxsize=None)
def proposal_inputs(name):
    """(params, base anchors (A, 4) float64, scores (1, 2A, H, W), deltas (1, 4A, H, W), im_info (1, 3)) of a case, float32 inputs."""
    c = dict(PROPOSALS[name])
    rng = np.random.default_rng(c["seed"])
    base = R.anchors(16, c["ratios"], c["scales"])
    a, h, w = len(base), c["H"], c["W"]
    m = h * w * a
    # foreground scores 1e-3 apart, in random places (the kernel takes any float: no two scores closer than MARGIN, ties planted on purpose)
    fg = (rng.permutation(m).astype(np.float64) + 1.0) * 1e-3
    if c.get("ties"):
        best = np.argsort(-fg)
        fg[best[3]] = fg[best[2]]
        fg[best[11]] = fg[best[10]] = fg[best[9]]
        fg[best[c["pre"]]] = fg[best[c["pre"] - 1]]                      # a tie across the pre_nms_topN cut
    scores = np.empty((1, 2 * a, h, w), np.float32)
    scores[0, a:] = fg.reshape(h, w, a).transpose(2, 0, 1)
    scores[0, :a] = rng.random((a, h, w))
    deltas = rng.normal(0, c.get("jitter", 0.25), (1, 4 * a, h, w))
    deltas[0, 0::4] *= c.get("shift", 1.0)
    deltas[0, 1::4] *= c.get("shift", 1.0)
    deltas[0, 2::4] = rng.normal(c["shrink"], 1.6 * c.get("jitter", 0.25), (a, h, w))
    deltas[0, 3::4] = rng.normal(c["shrink"], 1.6 * c.get("jitter", 0.25), (a, h, w))
    im_info = np.array([[h * FEAT_STRIDE, w * FEAT_STRIDE, 1.0]], np.float32)
    return c, base, scores, deltas.astype(np.float32), im_info


@functools.lru_cache(maxsize=None)
def proposal_reference(name):
    """(params, base, scores, deltas, im_info, result dict of ref_region64.proposal) - computed once, shared, never modified."""
    c, base, scores, deltas, im_info = proposal_inputs(name)
    out = R.proposal(scores, deltas, im_info, base, FEAT_STRIDE, c["pre"], c["post"], c["nms"], c["min_size"])
    return c, base, scores, deltas, im_info, out


# ---------------------------------------------------------------------------------------------------------------------- poolings
# ROIs as [image, x1, y1, x2, y2] in image pixels; the feature maps are N x C x 9 x 11 at spatial_scale 0.25 (a 36 x 44 image)
ROIS = np.array([
    [0, 4.0, 4.0, 27.0, 19.0],          # inside image 0: 7 x 5 cells
    [1, 3.0, 9.0, 30.2, 20.6],          # inside image 1
    [1, -13.0, -9.0, 52.0, 41.0],       # hangs over every edge
    [0, 17.0, 13.0, 17.5, 13.4],        # one cell: every bin of a larger pooled grid is that cell
    [0, 30.0, 26.0, 60.0, 47.0],        # over the right and lower edges: the far bins are empty
    [1, -40.0, -30.0, -21.0, -15.0],    # entirely outside: every bin is empty
    [0, 8.7, 0.0, 33.1, 35.0],
    [1, 0.0, 0.0, 43.0, 35.0],          # the whole image
], np.float32)
ROI_POOLS = {      # name -> (N, C, cstride, coffset, pooled_h, pooled_w)
    "c5_4x2": (2, 5, 8, 1, 4, 2),
    "c70_3x3": (2, 70, 72, 0, 3, 3),
    "c4_7x7": (2, 4, 4, 0, 7, 7),
}
POOL_H, POOL_W, POOL_SCALE = 9, 11, 0.25
# PSROIPooling at R-FCN's spatial_scale 0.0625: a 144 x 176 image over the same 9 x 11 map
PS_ROIS = np.array([
    [0, 16.0, 16.0, 99.0, 78.0],
    [1, 9.4, 30.2, 120.3, 100.1],
    [1, -50.0, -40.0, 210.0, 170.0],    # over every edge
    [0, 70.0, 52.0, 70.2, 52.3],        # one pixel: bins of 1 / 16 / group of a cell
    [0, 130.0, 110.0, 230.0, 190.0],    # over the right and lower edges
    [1, -160.0, -120.0, -84.0, -60.0],  # entirely outside
    [0, 0.0, 0.0, 175.0, 143.0],        # the whole image
    [1, 33.0, 5.0, 150.6, 139.0],
], np.float32)
PS_POOLS = {       # name -> (N, output_dim, group_size, cstride, coffset)
    "g3_d5": (2, 5, 3, 48, 2),
    "g7_d2": (2, 2, 7, 100, 0),
    "g7_d70": (2, 70, 7, 3430, 0),
}
PS_SCALE = 0.0625


@functools.lru_cache(maxsize=None)
def roi_pool_reference(name):
    n, c, _cs, _co, ph, pw = ROI_POOLS[name]
    x = np.random.default_rng(40 + c).standard_normal((n, c, POOL_H, POOL_W)).astype(np.float32)
    y, arg, margin = R.roi_pool(x, ROIS, ph, pw, POOL_SCALE)
    return x, y, arg, margin


@functools.lru_cache(maxsize=None)
def psroi_pool_reference(name):
    n, od, g, _cs, _co = PS_POOLS[name]
    x = np.random.default_rng(50 + od).standard_normal((n, od * g * g, POOL_H, POOL_W)).astype(np.float32)
    y, mag, largest, margin = R.psroi_pool(x, PS_ROIS, od, g, PS_SCALE)
    return x, y, mag, largest, margin


PAIR_SOFTMAX = {   # name -> (A, cstride, coffset, H, W)
    "a1": (1, 4, 0, 3, 5),
    "a9": (9, 20, 0, 5, 7),
    "a5_in_12": (5, 12, 0, 4, 3),
}
