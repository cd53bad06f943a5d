"""Inputs of the DetectionOutput cases that tests/test_gpu_guarded_ssd.py runs on the GPU, generated here so that the no-GPU margin
check (tests/test_ssd_ref.py) sees exactly the same arrays: a case whose float64 decisions are closer than MARGIN to a threshold
fails there, on the CPU, before any GPU time is spent.  The seeds were chosen so that every case holds the margin."""
import numpy as np

import ref_ssd64 as R

MARGIN = 1e-4       # two orders above the float32 rounding of a score or an overlap (about 1e-6)

# name -> parameters.  high: scores above the threshold per (image, class); empty: images without any; ties: plant equal scores;
# smother: a class whose candidates all sit on one box (the best one suppresses every other); small / spread: smaller boxes, fewer overlaps
CASES = {
    "p70_corner":       dict(P=70, classes=3, code=R.CORNER, var_enc=False, top_k=16, keep_top_k=-1, thr=0.25, nms=0.45, bg=0, high=40, seed=1),
    "p70_center_enc":   dict(P=70, classes=5, code=R.CENTER_SIZE, var_enc=True, top_k=-1, keep_top_k=9, thr=0.25, nms=0.45, bg=2, high=12, seed=2),
    "p300_center":      dict(P=300, classes=5, code=R.CENTER_SIZE, var_enc=False, top_k=16, keep_top_k=20, thr=0.25, nms=0.45, bg=0, high=40,
                             ties=True, seed=3),
    "p300_corner_enc":  dict(P=300, classes=3, code=R.CORNER, var_enc=True, top_k=-1, keep_top_k=30, thr=0.3, nms=0.3, bg=0, high=25,
                             smother=1, seed=4),
    "p300_one_empty":   dict(P=300, classes=3, code=R.CENTER_SIZE, var_enc=False, top_k=16, keep_top_k=8, thr=0.25, nms=0.45, bg=2, high=40,
                             empty=(1,), ties=True, seed=5),
    "p70_nothing":      dict(P=70, classes=3, code=R.CENTER_SIZE, var_enc=False, top_k=16, keep_top_k=10, thr=0.25, nms=0.45, bg=0, high=0, seed=6),
    "p2000_multipass":  dict(P=2000, classes=3, code=R.CENTER_SIZE, var_enc=False, top_k=200, keep_top_k=150, thr=0.25, nms=0.45, bg=0, high=1500,
                             small=True, seed=247),
    # top_k at the kernel's bound (the select kernel's sorted tile is full: 1024 candidates, four per thread) and more than 1024
    # survivors at the keep_top_k cut (its ranking streams two LDS tiles): small boxes spread over the image, few of which overlap
    "p1200_full_tile":  dict(P=1200, classes=4, N=1, code=R.CENTER_SIZE, var_enc=False, top_k=1024, keep_top_k=1100, thr=0.25, nms=0.45, bg=0,
                             high=1100, spread=True, seed=39),
    "ssd300_shape":     dict(P=8732, classes=21, N=1, code=R.CENTER_SIZE, var_enc=False, top_k=400, keep_top_k=200, thr=0.01, nms=0.45, bg=0, high=30,
                             seed=8),
    # ---- signed scores, no background, more than 256 classes (tests/test_ssd_ref.py asserts what each of them reaches)
    # scores as logits: 100 per (image, class) above a threshold of -4, 0.05 apart in -3.95 .. 0.5 (at most 30 rows of an image can be positive), every other one below it; the ties
    # of p300_center and one more lie among negative scores
    "logits":           dict(P=300, classes=4, code=R.CENTER_SIZE, var_enc=False, top_k=64, keep_top_k=40, thr=-4.0, nms=0.45, bg=0, high=90,
                             ties=True, logits=True, seed=9),
    # Caffe's default confidence_threshold: every prior of every class is a candidate; scores 0.01 apart, the best nine positive, then
    # the two zeros on two priors (one score: the lower prior index first), then negative ones
    "no_threshold":     dict(P=600, classes=3, code=R.CENTER_SIZE, var_enc=False, top_k=400, keep_top_k=200, thr=-float(np.finfo(np.float32).max),
                             nms=0.45, bg=0, high=0, ladder=590, seed=10),
    "no_background":    dict(P=70, classes=3, code=R.CORNER, var_enc=False, top_k=16, keep_top_k=-1, thr=0.25, nms=0.45, bg=-1, high=40, seed=11),
    # the per-image scan over the classes' counts runs two chunks of 256; image 1 has survivors in the second chunk only
    "c300":             dict(P=12, classes=300, code=R.CENTER_SIZE, var_enc=False, top_k=-1, keep_top_k=200, thr=0.25, nms=0.45, bg=150, high=2,
                             first_class={1: 256}, seed=12),
}
# cases that run a second time with `capacity` exactly what the images can yield (N * keep_top_k here) and the rows ending on the last byte
# in front of the red zone
EXACT_CAPACITY = ("p300_center", "p70_nothing")


def make(name):
    """(params, loc (N, P*4), conf (N, P*classes), priors (1, 2, P*4)) of a case, float32."""
    c = dict(CASES[name])
    c.setdefault("N", 2)
    rng = np.random.default_rng(c["seed"])
    p, nc, n = c["P"], c["classes"], c["N"]
    # priors in clusters, so that the NMS has overlaps to decide
    k = p if c.get("spread") else max(4, p // 12)
    centre = rng.uniform(0.1, 0.9, (k, 2))
    which = rng.integers(0, k, p)
    lo, hi = (0.01, 0.03) if c.get("spread") else (0.02, 0.06) if c.get("small") else (0.08, 0.3)
    cxy = centre[which] + rng.normal(0, 0.01 if c.get("small") else 0.03, (p, 2))
    wh = rng.uniform(lo, hi, (p, 2))
    boxes = np.concatenate([cxy - wh / 2, cxy + wh / 2], axis=1)
    priors = np.stack([boxes.reshape(-1), np.tile([0.1, 0.1, 0.2, 0.2], p)])[None].astype(np.float32)
    loc_scale = 1.0 if not c["var_enc"] or c["code"] == R.CENTER_SIZE else 0.05
    loc = (rng.normal(0, 0.3, (n, p * 4)) * loc_scale).astype(np.float32)
    smothered = rng.choice(p, min(c["high"], p), replace=False)
    if "smother" in c:
        pr = priors[0].reshape(2, p, 4)
        pr[:, smothered, :] = pr[:, smothered[0], :][:, None, :]
    thr = c["thr"]
    if c.get("ladder"):
        conf = np.empty((n, p, nc))
        for i in range(n):
            for cl in range(nc):
                step = rng.permutation(p)
                conf[i, :, cl] = (step - c["ladder"]) * 0.01
                conf[i, step == c["ladder"] - 1, cl] = -0.0
    elif c.get("logits"):
        conf = thr - 0.05 - np.abs(rng.normal(0.0, 3.0, (n, p, nc)))
    else:
        conf = rng.uniform(0.0, thr * 0.8, (n, p, nc))
    for i in range(n):
        if i in c.get("empty", ()):
            continue
        for cl in range(nc):
            if cl < c.get("first_class", {}).get(i, 0):
                continue
            at = rng.choice(p, min(c["high"], p), replace=False)
            if c.get("logits"):
                conf[i, at, cl] = thr + 0.05 * (1 + rng.permutation(at.size))
            else:
                conf[i, at, cl] = rng.uniform(thr + 0.05, 0.99, at.size)
            if c.get("smother") == cl and at.size:
                # every candidate of this class decodes to (nearly) the best one's box: the same priors in both images (the priors are
                # shared), the first of them with the best score, all on its prior and its loc
                at = smothered
                conf[i, :, cl] = rng.uniform(0.0, thr * 0.8, p)
                conf[i, at, cl] = rng.uniform(thr + 0.05, 0.9, at.size)
                conf[i, at[0], cl] = 0.95
                l4 = loc[i].reshape(p, 4)
                l4[at] = l4[at[0]] + (rng.normal(0, 0.01, (at.size, 4)) * loc_scale).astype(np.float32)
            if c.get("ties") and at.size > 20:
                srt = at[np.argsort(-conf[i, at, cl])]
                conf[i, srt[3], cl] = conf[i, srt[2], cl]                                  # a tie inside the kept range
                if c.get("logits"):
                    conf[i, srt[41], cl] = conf[i, srt[40], cl]                            # ... and one between two negative scores
                if c["top_k"] > 1:
                    conf[i, srt[c["top_k"]], cl] = conf[i, srt[c["top_k"] - 1], cl]          # a tie across the top_k cut
        if c.get("ties") and nc - (1 if c["bg"] >= 0 else 0) >= 2:
            a, b = [cl for cl in range(nc) if cl != c["bg"]][:2]
            conf[i, :, b] = conf[i, :, a]                                                    # two labels with the same scores: keep_top_k ties
    return c, loc, conf.astype(np.float32).reshape(n, p * nc), priors


def reference(name):
    """(params, loc, conf, priors, rows64, margin, count) of a case through the float64 reference."""
    c, loc, conf, priors = make(name)
    rows, margin, count = R.detection_output(loc, conf, priors, c["classes"], c["bg"], c["nms"], c["top_k"], c["code"], c["var_enc"],
                                             c["keep_top_k"], c["thr"])
    return c, loc, conf, priors, rows, margin, count
