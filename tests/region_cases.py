"""Inputs of the region-stage cases that tests/test_gpu_guarded_region.py runs on the GPU, generated here so that the no-GPU margin check
(tests/test_region_ref.py) sees exactly the same arrays: a case whose float64 decisions are closer than MARGIN to a threshold or to a
breakpoint fails there, on the CPU, before any GPU time is spent.  The seeds were chosen so that every case holds the margin."""
import functools

import numpy as np

import ref_region64 as R

MARGIN = 1e-4       # the SSD tests' figure: two orders above the float32 rounding of a score, an overlap or a bin edge

SMALL = dict(ratios=(0.5, 1.0, 2.0), scales=(1.0, 2.0, 4.0))      # 16 .. 64 pixel anchors for the small maps
# name -> parameters.  The image is (H, W) * feat_stride at scale 1 unless `im` (height, width, scale) says otherwise; shrink: mean of
# dw / dh (negative: boxes smaller than their anchors); jitter: the deltas' spread (small: neighbouring anchors decode to boxes that
# overlap); ties: plant equal scores among the best
PROPOSALS = {
    "m5x7":         dict(H=5, W=7, pre=100, post=20, nms=0.7, min_size=16, shrink=0.3, jitter=0.05, seed=1, **SMALL),
    "m12x10_tiles": dict(H=12, W=10, pre=150, post=60, nms=0.5, min_size=24, shrink=0.2, jitter=0.05, seed=2, ties=True, **SMALL),
    "filter_clip":  dict(H=5, W=7, pre=100, post=30, nms=0.7, min_size=24, shrink=-0.7, shift=1.5, seed=3, **SMALL),
    "few_survive":  dict(H=3, W=4, pre=100, post=40, nms=0.3, min_size=16, shrink=0.3, seed=4, **SMALL),
    "post_cut":     dict(H=5, W=7, pre=100, post=5, nms=0.7, min_size=16, shrink=-0.3, seed=5, **SMALL),
    "pre_above":    dict(H=5, W=7, pre=6000, post=50, nms=0.5, min_size=16, shrink=0.0, seed=6, **SMALL),
    "rfcn_full":    dict(H=38, W=63, pre=6000, post=300, nms=0.7, min_size=16, shrink=-0.5, jitter=0.1, seed=7, ratios=(0.5, 1.0, 2.0),
                         scales=(8.0, 16.0, 32.0)),
    # ---- the cases below walk what the seven above never reach (tests/test_region_ref.py asserts, case by case, that they do)
    # nms_thresh 1.0: no overlap exceeds it, every place of every word is kept (K = 4356, 69 words); its twin at -1.0: every pair
    # suppresses, pairs of overlap 0 included, and one box is left
    "keep_everything": dict(H=22, W=22, pre=6144, post=6144, nms=1.0, min_size=0, shrink=0.0, seed=11, **SMALL),
    "suppress_everything": dict(H=22, W=22, pre=6144, post=6144, nms=-1.0, min_size=0, shrink=0.0, seed=11, **SMALL),
    # FCN_PROPOSAL_MAX_CANDIDATES: eight ranking slices of four full LDS tiles; equal scores on both sides of a tile and of a slice boundary
    "max_candidates": dict(H=64, W=64, pre=6000, post=300, nms=0.7, min_size=16, shrink=-0.1, jitter=0.1, seed=12, ratios=(3.0, 2.0, 1.0, 0.5),
                           scales=(2.0, 4.0, 8.0, 16.0), tie_pairs=((2047, 2048), (8191, 8192))),
    "a32":          dict(H=3, W=5, pre=300, post=40, nms=0.6, min_size=16, shrink=0.0, seed=13, ratios=(0.5, 1.0, 2.0, 3.0),
                         scales=(1.0, 1.5, 2.0, 2.5, 3.0, 3.5, 4.0, 5.0)),
    "a1":           dict(H=7, W=9, pre=100, post=30, nms=0.3, min_size=16, shrink=0.2, seed=14, ratios=(1.0,), scales=(2.0,)),
    "one":          dict(H=1, W=1, pre=1, post=1, nms=0.7, min_size=8, shrink=0.0, seed=15, ratios=(1.0,), scales=(1.0,), im=(32, 32, 1.0)),
    "one_filtered": dict(H=1, W=1, pre=1, post=1, nms=0.7, min_size=16, shrink=-1.0, seed=15, ratios=(1.0,), scales=(1.0,), im=(32, 32, 1.0)),
    "none_survive": dict(H=5, W=7, pre=100, post=20, nms=0.7, min_size=16, shrink=-4.0, seed=16, **SMALL),
    # an image smaller than the map's extent and a scale that is not 1: the bound is 25.6 pixels and the clip is the image's
    "scaled_image": dict(H=5, W=7, pre=100, post=30, nms=0.7, min_size=16, shrink=-0.2, shift=1.5, seed=17, im=(5 * 16 - 37, 7 * 16 - 21, 1.6),
                         **SMALL),
    "signed_scores": dict(H=5, W=7, pre=400, post=315, nms=0.7, min_size=16, shrink=0.3, jitter=0.05, seed=18, signed=True, **SMALL),
    # m5x7 with a NaN in five scores and in one delta of five other candidates; the second one without a size bound to hide behind
    "nan_inputs":   dict(H=5, W=7, pre=100, post=20, nms=0.7, min_size=16, shrink=0.3, jitter=0.05, seed=1, nan=True, **SMALL),
    "nan_min0":     dict(H=5, W=7, pre=100, post=20, nms=0.7, min_size=0, shrink=0.3, jitter=0.05, seed=1, nan=True, **SMALL),
    # ---- the placed generator (below): the decoded box of every candidate is chosen, the deltas follow
    "deep_sweep":   dict(H=24, W=24, pre=6144, post=300, nms=0.7, min_size=16, seed=21, placed=dict(lead=100, dup_until=4300), im=(700, 700, 1.0),
                         **SMALL),
    "pre_6144":     dict(H=26, W=27, pre=6144, post=300, nms=0.7, min_size=16, seed=22, placed=dict(lead=100, dup_until=5900, force=(6143, 6144)),
                         im=(700, 700, 1.0), **SMALL),
}
FEAT_STRIDE = 16
SITE, PITCH, SITE_OFFSET, P_NEW = 24, 30, 4, 0.45


def _layout(c, base, fg, dl):
    """Candidate-major scores (m,) and deltas (m, 4), float64 -> the float32 blobs and im_info."""
    a, h, w = len(base), c["H"], c["W"]
    rng = np.random.default_rng(c["seed"] + 5000)
    scores = np.empty((1, 2 * a, h, w), np.float32)
    scores[0, a:] = fg.reshape(h, w, a).transpose(2, 0, 1)
    scores[0, :a] = rng.random((a, h, w))
    deltas = np.ascontiguousarray(dl.reshape(h, w, a, 4).transpose(2, 3, 0, 1)).reshape(1, 4 * a, h, w)
    im_info = np.array([c.get("im", (h * FEAT_STRIDE, w * FEAT_STRIDE, 1.0))], np.float32)
    return scores, deltas.astype(np.float32), im_info


def placed_inputs(c, base):
    """The generator that places boxes on purpose.  Independent random boxes fill post_nms_topn within a few hundred places of the order;
    here the decoded box of every candidate is chosen and the decode is inverted in float64 (dx = (tcx - acx) / aw, dw = log(tw / aw),
    y likewise; the float32 cast of those deltas is the input, which the reference consumes like the kernel).

    Boxes live on disjoint SITEs: squares of 24 pixels at a pitch of 30, each box at its site with +-0.5 pixels of jitter in every
    corner.  Two boxes of one site overlap at about 0.85 (>= 0.84), two of different sites at 0: every comparison of the NMS is far from
    0.7.  The first box of a site in the order (its leader) is kept, every later one (a duplicate) is suppressed by it.  Place p of the order
    holds: for p < lead a new site's leader; up to dup_until a duplicate of a site seen so far; from there on (and at the places in `force`)
    a new leader with probability 0.45, else a duplicate.  Scores fall by 1e-3 a place and are shifted so that half of them are negative and
    none is zero; place -> candidate is a random permutation, so the order has nothing to do with the order in memory.  Every box lies
    inside the image (the corner tolerance's derivation asks for that)."""
    p = c["placed"]
    rng = np.random.default_rng(c["seed"])
    a, h, w = len(base), c["H"], c["W"]
    m = h * w * a
    im_h, im_w, _scale = c["im"]
    nx, ny = (im_w - SITE - 1 - SITE_OFFSET) // PITCH + 1, (im_h - SITE - 1 - SITE_OFFSET) // PITCH + 1
    unseen = list(rng.permutation(nx * ny))
    seen, site = [], np.empty(m, np.int64)
    for place in range(m):
        coin, pick = rng.random(), rng.random()
        new = place < p["lead"] or place in p.get("force", ()) or (place >= p["dup_until"] and coin < P_NEW)
        if new and unseen:
            seen.append(unseen.pop())
            site[place] = seen[-1]
        else:
            site[place] = seen[int(pick * len(seen))]
    x0, y0 = SITE_OFFSET + PITCH * (site % nx), SITE_OFFSET + PITCH * (site // nx)
    jit = rng.uniform(-0.5, 0.5, (m, 4))
    target = np.stack([x0, y0, x0 + SITE - 1, y0 + SITE - 1], axis=1) + jit          # by place
    score = (m / 2 - np.arange(m) - 0.5) * 1e-3
    if c["pre"] < m:
        score[c["pre"]] = score[c["pre"] - 1]                                        # a tie across the pre_nms_topN cut
    cand = rng.permutation(m)                                                        # place -> candidate
    box, fg = np.empty((m, 4)), np.empty(m)
    box[cand], fg[cand] = target, score
    anc = R.all_anchors(base, h, w, FEAT_STRIDE)
    aw, ah = anc[:, 2] - anc[:, 0] + 1, anc[:, 3] - anc[:, 1] + 1
    acx, acy = anc[:, 0] + 0.5 * aw, anc[:, 1] + 0.5 * ah
    dl = np.stack([(0.5 * (box[:, 0] + box[:, 2]) - acx) / aw, (0.5 * (box[:, 1] + box[:, 3]) - acy) / ah,
                   np.log((box[:, 2] - box[:, 0]) / aw), np.log((box[:, 3] - box[:, 1]) / ah)], axis=1)
    return _layout(c, base, fg, dl)


def _signed(c, base, scores, deltas, im_info):
    """New values for the scores of a case, place by place of the order they have, so that the order (and with it what the NMS keeps) stays:
    +inf at place 0, then positive scores 1e-3 apart, three positive denormals, four zeros of alternating sign (one score: they go by
    candidate index), three negative denormals, negative scores, and -inf from the last kept place on.  The zero crossing is put at the
    first place where a denormal of each sign and a zero of each sign are rows of the result."""
    a, h, w = len(base), c["H"], c["W"]
    first = R.proposal(scores, deltas, im_info, base, FEAT_STRIDE, c["pre"], c["post"], c["nms"], c["min_size"])
    order, n, last = first["order"], len(first["order"]), first["places"][-1]
    fg0 = scores[0, a:].transpose(1, 2, 0).reshape(-1).astype(np.float64)
    tiny = float(np.float32(1e-40))
    for z in range(8, last - 8):
        v = np.empty(n)
        v[:z - 3] = (z - 3 - np.arange(z - 3)) * 1e-3
        v[z - 3:z] = [3 * tiny, 2 * tiny, tiny]
        zeros = np.sort(order[z:z + 4])
        v[z + 4:z + 7] = [-tiny, -2 * tiny, -3 * tiny]
        v[z + 7:] = -(np.arange(z + 7, n) - z - 6) * 1e-3
        v[0], v[last:] = np.inf, -np.inf
        fg = fg0.copy()
        fg[order] = v
        fg[zeros] = [-0.0, 0.0, -0.0, 0.0]
        out = scores.copy()
        out[0, a:] = fg.reshape(h, w, a).transpose(2, 0, 1)
        rows = R.proposal(out, deltas, im_info, base, FEAT_STRIDE, c["pre"], c["post"], c["nms"], c["min_size"], score_gaps=False)
        s = rows["scores"][:rows["count"], 0]
        if (np.any((s > 0) & (s < 1e-38)) and np.any((s < 0) & (s > -1e-38)) and np.any((s == 0) & np.signbit(s)) and
                np.any((s == 0) & ~np.signbit(s))):
            return out
    raise AssertionError("no zero crossing of case signed_scores puts every special score among the rows")


def _nan(c, base, scores, deltas, im_info):
    """NaN into five scores and into one delta (dx, dy, dw, dh, dw) of five other candidates, chosen from what the case gives without them:
    rows 0, 4 and 9 and the first two boxes that are no rows (suppressed ones, then the next of the order) lose their score; rows 2, 6
    and 12, the third such box and the first candidate of the map a delta."""
    a = len(base)
    clean = R.proposal(scores, deltas, im_info, base, FEAT_STRIDE, c["pre"], c["post"], c["nms"], c["min_size"])
    dropped = [int(clean["order"][p]) for p, _by in clean["suppressors"]] + [int(i) for i in clean["order"][depth(clean):]]      # (then the next of the order)
    no_score = [clean["index"][0], clean["index"][4], clean["index"][9]] + dropped[:2]
    no_delta = [clean["index"][2], clean["index"][6], clean["index"][12], dropped[2], 0]
    assert len(set(no_score + no_delta)) == 10
    scores, deltas = scores.copy(), deltas.copy()
    for i in no_score:
        pix, k = divmod(i, a)
        scores[0, a + k, pix // c["W"], pix % c["W"]] = np.nan
    for i, comp in zip(no_delta, (0, 1, 2, 3, 2)):
        pix, k = divmod(i, a)
        deltas[0, 4 * k + comp, pix // c["W"], pix % c["W"]] = np.nan
    return scores, deltas, tuple(no_score), tuple(no_delta), clean


@functools.lru_cache(maxsize=None)
def proposal_inputs(name):
    """(params, base anchors (A, 4) float64, scores (1, 2A, H, W), deltas (1, 4A, H, W), im_info (1, 3)) of a case, float32 inputs."""
    c = dict(PROPOSALS[name])
    base = R.anchors(16, c["ratios"], c["scales"])
    if "placed" in c:
        return (c, base) + placed_inputs(c, base)
    c, base, scores, deltas, im_info = _random_inputs(c, base)
    if c.get("signed"):
        scores = _signed(c, base, scores, deltas, im_info)
    if c.get("nan"):
        scores, deltas, c["no_score"], c["no_delta"], c["clean"] = _nan(c, base, scores, deltas, im_info)
    return c, base, scores, deltas, im_info


def _random_inputs(c, base):
    rng = np.random.default_rng(c["seed"])
    a, h, w = len(base), c["H"], c["W"]
    m = h * w * a
    # foreground scores 1e-3 apart, in random places (the kernel takes any float: no two scores closer than MARGIN, ties planted on purpose)
    fg = (rng.permutation(m).astype(np.float64) + 1.0) * 1e-3
    if c.get("ties"):
        best = np.argsort(-fg)
        fg[best[3]] = fg[best[2]]
        fg[best[11]] = fg[best[10]] = fg[best[9]]
        fg[best[c["pre"]]] = fg[best[c["pre"] - 1]]                      # a tie across the pre_nms_topN cut
    for rank, (i, j) in enumerate(c.get("tie_pairs", ())):               # equal scores at two given candidates, above every other score
        fg[i] = fg[j] = (m + len(c["tie_pairs"]) - rank) * 1e-3
    scores = np.empty((1, 2 * a, h, w), np.float32)
    scores[0, a:] = fg.reshape(h, w, a).transpose(2, 0, 1)
    scores[0, :a] = rng.random((a, h, w))
    deltas = rng.normal(0, c.get("jitter", 0.25), (1, 4 * a, h, w))
    deltas[0, 0::4] *= c.get("shift", 1.0)
    deltas[0, 1::4] *= c.get("shift", 1.0)
    deltas[0, 2::4] = rng.normal(c["shrink"], 1.6 * c.get("jitter", 0.25), (a, h, w))
    deltas[0, 3::4] = rng.normal(c["shrink"], 1.6 * c.get("jitter", 0.25), (a, h, w))
    for i, j in c.get("tie_pairs", ()):                                  # ... whose boxes are their anchors: alive, and far from each other
        for cand in (i, j):
            pix, k = divmod(cand, a)
            deltas[0, 4 * k:4 * k + 4, pix // w, pix % w] = 0.0
    im_info = np.array([c.get("im", (h * FEAT_STRIDE, w * FEAT_STRIDE, 1.0))], np.float32)
    return c, base, scores, deltas.astype(np.float32), im_info


@functools.lru_cache(maxsize=None)
def proposal_reference(name):
    """(params, base, scores, deltas, im_info, result dict of ref_region64.proposal) - computed once, shared, never modified.
    signed_scores is the one case whose score gaps stay out of the margin: its scores are compared as they are and their spacing -
    denormals beside the zeros - is what it is about (ref_region64.proposal, score_gaps)."""
    c, base, scores, deltas, im_info = proposal_inputs(name)
    out = R.proposal(scores, deltas, im_info, base, FEAT_STRIDE, c["pre"], c["post"], c["nms"], c["min_size"], score_gaps=not c.get("signed"))
    return c, base, scores, deltas, im_info, out


def depth(out):
    """The last place of the order that the greedy NMS looks at: the boxes it kept and the ones it dropped before it stopped."""
    return out["count"] + out["suppressed"]


def decode32(c, base, deltas, im_info):
    """The decode and the clip of every candidate in numpy float32, one rounding an operation and no contraction, in the order of
    operations the contract gives: what a float32 implementation computes, against which the corner tolerance is justified."""
    f = np.float32
    a, h, w = len(base), c["H"], c["W"]
    anc = R.all_anchors(base, h, w, FEAT_STRIDE).astype(f)
    d = deltas[0].reshape(a, 4, h, w).transpose(2, 3, 0, 1).reshape(-1, 4).astype(f)
    bw, bh = anc[:, 2] - anc[:, 0] + f(1), anc[:, 3] - anc[:, 1] + f(1)
    cx, cy = anc[:, 0] + f(0.5) * bw, anc[:, 1] + f(0.5) * bh
    with np.errstate(invalid="ignore", over="ignore"):
        pcx, pcy = d[:, 0] * bw + cx, d[:, 1] * bh + cy
        pw, ph = np.exp(d[:, 2]) * bw, np.exp(d[:, 3]) * bh
        box = np.stack([pcx - f(0.5) * pw, pcy - f(0.5) * ph, pcx + f(0.5) * pw, pcy + f(0.5) * ph], axis=1)
    assert box.dtype == f
    box[:, 0::2] = np.clip(box[:, 0::2], f(0), im_info[0, 1] - f(1))
    box[:, 1::2] = np.clip(box[:, 1::2], f(0), im_info[0, 0] - f(1))
    return box


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
