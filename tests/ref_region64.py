"""Float64 restatement of the region stage of the two-stage detectors, written from the layers' definitions and without reading the
package: the anchors and the Proposal layer of py-faster-rcnn (TEST settings), ROIPooling, R-FCN's PSROIPooling and the RPN's two-class
softmax.  Blobs are NCHW.

Like tests/ref_ssd64.py every function that decides something also returns the MARGIN of its decisions:
  proposal   the smallest gap between two neighbouring, distinct scores of the order (the pre_nms_topN cut is the gap between two such
             neighbours), the smallest |overlap - nms_thresh| over every comparison the greedy NMS makes, and the smallest distance of a
             box extent from the min_size bound (a candidate with a NaN score or a NaN corner is no candidate and has no extent to
             measure);
  poolings   the smallest distance of an argument of round / floor / ceil from a breakpoint of that function.  An argument that float32
             arithmetic (IEEE, no contraction) computes to the very same value as float64 is decided alike in both formats whatever its
             distance and is left out: 0.0625 * 32, 1.25 * 4 and (1 / 3) * 3 are such values.
A float32 kernel whose scores, overlaps and bin edges are off by rounding decides as this file does when the margin is well above that
rounding; the tests assert the margin on their inputs before they compare."""
import numpy as np

F64 = np.float64


def anchors(base_size=16, ratios=(0.5, 1.0, 2.0), scales=(8.0, 16.0, 32.0)):
    """(A, 4) float64, ratio-major, scale-minor."""
    w = h = float(base_size)
    c = 0.5 * (base_size - 1)
    out = []
    for r in ratios:
        ws = np.round(np.sqrt(w * h / r))       # numpy's round: halves to even
        hs = np.round(ws * r)
        for s in scales:
            bw, bh = ws * s, hs * s
            out.append([c - 0.5 * (bw - 1), c - 0.5 * (bh - 1), c + 0.5 * (bw - 1), c + 0.5 * (bh - 1)])
    return np.array(out, F64)


def all_anchors(base, h, w, feat_stride):
    """(h * w * A, 4): candidate (y w + x) A + a is anchor a shifted by (x, y) * feat_stride."""
    ys, xs = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    shift = np.stack([xs, ys, xs, ys], axis=-1).reshape(-1, 1, 4) * float(feat_stride)
    return (np.asarray(base, F64)[None] + shift).reshape(-1, 4)


def decode(anchor_boxes, deltas):
    a, d = np.asarray(anchor_boxes, F64), np.asarray(deltas, F64)
    w, h = a[:, 2] - a[:, 0] + 1, a[:, 3] - a[:, 1] + 1
    cx, cy = a[:, 0] + 0.5 * w, a[:, 1] + 0.5 * h
    pcx, pcy = d[:, 0] * w + cx, d[:, 1] * h + cy
    pw, ph = np.exp(d[:, 2]) * w, np.exp(d[:, 3]) * h
    return np.stack([pcx - 0.5 * pw, pcy - 0.5 * ph, pcx + 0.5 * pw, pcy + 0.5 * ph], axis=1)


def overlaps(b, others):
    """The +1 overlap of box b with each row of `others`."""
    b, o = np.asarray(b, F64), np.asarray(others, F64).reshape(-1, 4)
    area = lambda q: (q[..., 2] - q[..., 0] + 1) * (q[..., 3] - q[..., 1] + 1)
    iw = np.maximum(0.0, np.minimum(b[2], o[:, 2]) - np.maximum(b[0], o[:, 0]) + 1)
    ih = np.maximum(0.0, np.minimum(b[3], o[:, 3]) - np.maximum(b[1], o[:, 1]) + 1)
    inter = iw * ih
    return inter / (area(b) + area(o) - inter)


def proposal(scores, deltas, im_info, base_anchors, feat_stride=16, pre_nms_topn=6000, post_nms_topn=300, nms_thresh=0.7, min_size=16,
             score_gaps=True):
    """scores (1, 2A, H, W), deltas (1, 4A, H, W), im_info (1, 3) or (3,) -> dict with
    rois (post_nms_topn, 5) float64 (rows at and past `count` are zeros), scores (post_nms_topn, 1), count, index (the candidates of the
    rows, in order), suppressed (boxes the NMS dropped before it stopped), filtered (candidates the size filter dropped), margin; and for
    the tests that say which path a case walks: order (the candidates that went into the NMS, place by place), places (the place of each
    row's candidate in that order), suppressors ((place of a dropped box, place of the kept box that dropped it) for each dropped box),
    raw (the boxes before the clip), boxes (after it) and alive (the candidates that pass step 3).

    A NaN is no number to compare: a candidate whose score is a NaN, or whose box has a NaN corner (a NaN delta), is not alive - it is
    counted in `filtered` - and the min_size margin is taken over the other candidates only.

    score_gaps=False leaves the gaps between neighbouring scores out of the margin.  It is for inputs whose scores are the layer's own
    bottom and are compared as they are, bit for bit, with no arithmetic in front of the comparison that could round: a case that is about
    the spacing of the floats themselves (denormals beside the two zeros) then keeps a margin over what IS computed - extents and overlaps."""
    scores, deltas = np.asarray(scores, F64), np.asarray(deltas, F64)
    im = np.asarray(im_info, F64).reshape(-1)
    assert scores.shape[0] == 1 and deltas.shape[0] == 1
    base = np.asarray(base_anchors, F64)
    a = base.shape[0]
    _, c2, h, w = scores.shape
    assert c2 == 2 * a and deltas.shape == (1, 4 * a, h, w)
    fg = scores[0, a:].transpose(1, 2, 0).reshape(-1)                      # (y, x, a) order
    dl = deltas[0].reshape(a, 4, h, w).transpose(2, 3, 0, 1).reshape(-1, 4)
    with np.errstate(invalid="ignore", over="ignore"):
        raw = decode(all_anchors(base, h, w, feat_stride), dl)
    number = ~(np.isnan(fg) | np.isnan(raw).any(axis=1))
    boxes = raw.copy()
    boxes[:, 0::2] = np.clip(boxes[:, 0::2], 0.0, im[1] - 1)
    boxes[:, 1::2] = np.clip(boxes[:, 1::2], 0.0, im[0] - 1)
    bound = min_size * im[2]
    ext = np.stack([boxes[:, 2] - boxes[:, 0] + 1, boxes[:, 3] - boxes[:, 1] + 1], axis=1)
    margin = float(np.min(np.abs(ext[number] - bound))) if number.any() else np.inf
    with np.errstate(invalid="ignore"):
        alive = np.nonzero(number & (ext[:, 0] >= bound) & (ext[:, 1] >= bound))[0]
    order = alive[np.lexsort((alive, -fg[alive]))]                        # score descending, ties by candidate index ascending
    # every neighbouring pair of the order up to and across the cut
    upto = min(len(order), pre_nms_topn + 1)
    with np.errstate(invalid="ignore"):
        gaps = -np.diff(fg[order[:upto]])                                 # (two infinities of one sign: a NaN, which is no gap)
    gaps = gaps[gaps > 0]
    if gaps.size and score_gaps:
        margin = min(margin, float(gaps.min()))
    order = order[:pre_nms_topn]
    kept, places, suppressors = [], [], []
    for place, i in enumerate(order):
        if len(kept) == post_nms_topn:
            break
        if kept:
            ov = overlaps(boxes[i], boxes[kept])
            over = np.nonzero(ov > nms_thresh)[0]
            seen = ov if over.size == 0 else ov[:over[0] + 1]          # the greedy loop stops at the first box that suppresses
            margin = min(margin, float(np.min(np.abs(seen - nms_thresh))))
            if over.size:
                suppressors.append((place, places[over[0]]))
                continue
        kept.append(int(i))
        places.append(place)
    rois = np.zeros((post_nms_topn, 5), F64)
    sc = np.zeros((post_nms_topn, 1), F64)
    rois[:len(kept), 1:] = boxes[kept]
    sc[:len(kept), 0] = fg[kept]
    return dict(rois=rois, scores=sc, count=len(kept), index=kept, suppressed=len(suppressors), filtered=int(fg.size - alive.size),
                margin=margin, boxes=boxes, raw=raw, alive=alive, order=order, places=places, suppressors=suppressors)


# ---------------------------------------------------------------------------------------------------------------------- poolings
def c_round(v):
    """C's round: halves away from zero."""
    return np.sign(v) * np.floor(np.abs(v) + 0.5)


class _Margin:
    """Collects the distance of each rounding argument from its function's breakpoint; an argument that the float32 evaluation reproduces
    bit for bit is left out."""

    def __init__(self):
        self.value = np.inf

    def see(self, kind, v64, v32):
        if float(v32) == float(v64):
            return
        frac = float(v64) - np.floor(float(v64))
        d = abs(frac - 0.5) if kind == "round" else min(frac, 1.0 - frac)
        self.value = min(self.value, d)


def _roi_bins(roi, scale, ph_n, pw_n, T):
    """ROIPooling's bin edges before clipping, in arithmetic of type T: (args, hstart[], hend[], wstart[], wend[]) where args lists every
    (kind, argument) that was rounded, in a fixed order."""
    args = []

    def rnd(v):
        args.append(("round", v))
        return int(c_round(F64(v)))

    def flo(v):
        args.append(("floor", v))
        return int(np.floor(F64(v)))

    def cei(v):
        args.append(("ceil", v))
        return int(np.ceil(F64(v)))

    r = [T(v) for v in roi]
    s = T(scale)
    sw, sh, ew, eh = rnd(r[1] * s), rnd(r[2] * s), rnd(r[3] * s), rnd(r[4] * s)
    roi_w, roi_h = max(ew - sw + 1, 1), max(eh - sh + 1, 1)
    bin_h, bin_w = T(roi_h) / T(ph_n), T(roi_w) / T(pw_n)
    hs = [flo(T(p) * bin_h) + sh for p in range(ph_n)]
    he = [cei(T(p + 1) * bin_h) + sh for p in range(ph_n)]
    ws = [flo(T(p) * bin_w) + sw for p in range(pw_n)]
    we = [cei(T(p + 1) * bin_w) + sw for p in range(pw_n)]
    return args, hs, he, ws, we


def _psroi_bins(roi, scale, g, T):
    args = []

    def rnd(v):
        args.append(("round", v))
        return T(c_round(F64(v)))

    def flo(v):
        args.append(("floor", v))
        return int(np.floor(F64(v)))

    def cei(v):
        args.append(("ceil", v))
        return int(np.ceil(F64(v)))

    r = [T(v) for v in roi]
    s = T(scale)
    sw, sh = rnd(r[1]) * s, rnd(r[2]) * s
    ew, eh = (rnd(r[3]) + T(1)) * s, (rnd(r[4]) + T(1)) * s
    roi_w, roi_h = max(ew - sw, T(0.1)), max(eh - sh, T(0.1))
    bin_h, bin_w = roi_h / T(g), roi_w / T(g)
    hs = [flo(T(p) * bin_h + sh) for p in range(g)]
    he = [cei(T(p + 1) * bin_h + sh) for p in range(g)]
    ws = [flo(T(p) * bin_w + sw) for p in range(g)]
    we = [cei(T(p + 1) * bin_w + sw) for p in range(g)]
    return args, hs, he, ws, we


def _edges(fn, m, *a):
    a64 = fn(*a, F64)
    a32 = fn(*a, np.float32)
    for (kind, v64), (_k, v32) in zip(a64[0], a32[0]):
        m.see(kind, v64, v32)
    return a64[1:]


def roi_pool(x, rois, pooled_h, pooled_w, spatial_scale):
    """x (N, C, H, W), rois (R, 5) -> (y (R, C, pooled_h, pooled_w) float64, argmax (same shape, int: h * W + w or -1), margin)."""
    x = np.asarray(x, F64)
    n, c, h, w = x.shape
    rois = np.asarray(rois, F64)
    y = np.zeros((len(rois), c, pooled_h, pooled_w), F64)
    arg = np.full(y.shape, -1, np.int64)
    m = _Margin()
    for r, roi in enumerate(rois):
        b = int(roi[0])
        hs, he, ws, we = _edges(_roi_bins, m, roi, spatial_scale, pooled_h, pooled_w)
        for ph in range(pooled_h):
            for pw in range(pooled_w):
                h0, h1 = min(max(hs[ph], 0), h), min(max(he[ph], 0), h)
                w0, w1 = min(max(ws[pw], 0), w), min(max(we[pw], 0), w)
                if h1 <= h0 or w1 <= w0:
                    continue
                win = x[b, :, h0:h1, w0:w1].reshape(c, -1)
                at = np.argmax(win, axis=1)                         # (the first maximum in raster order)
                y[r, :, ph, pw] = win[np.arange(c), at]
                arg[r, :, ph, pw] = (h0 + at // (w1 - w0)) * w + w0 + at % (w1 - w0)
    return y, arg, m.value


def psroi_pool(x, rois, output_dim, group_size, spatial_scale):
    """x (N, output_dim * group_size^2, H, W), rois (R, 5) -> (y (R, output_dim, g, g) float64, mean |x| over each bin (the magnitude term
    of the sum's allowance), largest bin in pixels, margin)."""
    x = np.asarray(x, F64)
    n, c, h, w = x.shape
    g = group_size
    assert c == output_dim * g * g
    rois = np.asarray(rois, F64)
    y = np.zeros((len(rois), output_dim, g, g), F64)
    mag = np.zeros_like(y)
    m = _Margin()
    largest = 0
    for r, roi in enumerate(rois):
        b = int(roi[0])
        hs, he, ws, we = _edges(_psroi_bins, m, roi, spatial_scale, g)
        for ph in range(g):
            for pw in range(g):
                h0, h1 = min(max(hs[ph], 0), h), min(max(he[ph], 0), h)
                w0, w1 = min(max(ws[pw], 0), w), min(max(we[pw], 0), w)
                if h1 <= h0 or w1 <= w0:
                    continue
                largest = max(largest, (h1 - h0) * (w1 - w0))
                ch = (np.arange(output_dim) * g + ph) * g + pw
                win = x[b, ch, h0:h1, w0:w1].reshape(output_dim, -1)
                y[r, :, ph, pw] = win.mean(axis=1)
                mag[r, :, ph, pw] = np.abs(win).mean(axis=1)
    return y, mag, largest, m.value


def pair_softmax(x):
    """Reshape(0, 2, -1, 0) -> Softmax(axis 1) -> Reshape(0, 2A, -1, 0) of (N, 2A, H, W): channel pairs (a, a + A)."""
    x = np.asarray(x, F64)
    n, c2, h, w = x.shape
    v = x.reshape(n, 2, (c2 // 2) * h, w)
    e = np.exp(v - v.max(axis=1, keepdims=True))
    return (e / e.sum(axis=1, keepdims=True)).reshape(n, c2, h, w)
