"""Float64 restatement of the SSD detection head (Caffe-SSD's layers, as remembered), written from their definitions and without
reading the package: PriorBox, Normalize, the Permute + Flatten + Concat gather, the row softmax and DetectionOutput.

detection_output also returns the MARGIN of its own decisions - the smallest of |score - confidence_threshold| over every (prior,
class), |overlap - nms_threshold| over every comparison the NMS makes, and the gap between the two adjacent distinct scores at every
top_k / keep_top_k cut.  A float32 kernel whose scores and overlaps are off by rounding decides as this file does when the margin is
well above that rounding; the tests assert the margin on their inputs before they compare."""
import math

import numpy as np

F64 = np.float64
CORNER, CENTER_SIZE = 1, 2


def expand_ratios(aspect_ratios, flip=True):
    out = [1.0]
    for ar in aspect_ratios:
        for v in ([ar, 1.0 / ar] if flip else [ar]):
            if all(abs(v - o) >= 1e-6 for o in out):
                out.append(v)
    return out


def prior_box(fh, fw, img_h, img_w, min_sizes, max_sizes=(), aspect_ratios=(), flip=True, clip=False, variance=(0.1,), step=None, offset=0.5):
    """(1, 2, fh * fw * A * 4) float64.  step: None (image extent / map extent), a number, or (step_h, step_w)."""
    if max_sizes and len(max_sizes) != len(min_sizes):
        raise ValueError("max_size count")
    if any(m <= s for s, m in zip(min_sizes, max_sizes)):
        raise ValueError("max_size <= min_size")
    if len(variance) not in (1, 4):
        raise ValueError("variance count")
    ratios = expand_ratios(aspect_ratios, flip)
    step_h, step_w = (img_h / fh, img_w / fw) if step is None else (step if isinstance(step, tuple) else (step, step))
    boxes = []
    for h in range(fh):
        for w in range(fw):
            cx, cy = (w + offset) * step_w, (h + offset) * step_h
            for i, s in enumerate(min_sizes):
                sizes = [(s, s)]
                if max_sizes:
                    q = math.sqrt(s * max_sizes[i])
                    sizes.append((q, q))
                sizes += [(s * math.sqrt(ar), s / math.sqrt(ar)) for ar in ratios if abs(ar - 1.0) >= 1e-6]
                for bw, bh in sizes:
                    boxes.append([(cx - bw / 2) / img_w, (cy - bh / 2) / img_h, (cx + bw / 2) / img_w, (cy + bh / 2) / img_h])
    b = np.array(boxes, F64)
    if clip:
        b = np.clip(b, 0.0, 1.0)
    var = np.tile(np.array(list(variance) * (4 if len(variance) == 1 else 1), F64), len(boxes))
    return np.stack([b.reshape(-1), var])[None]


def normalize(x, scale, eps=1e-10):
    """x (N, C, H, W); scale (C,) or (1,): y = scale * x / sqrt(sum_c x^2 + eps) per pixel."""
    x = np.asarray(x, F64)
    s = np.asarray(scale, F64).reshape(-1)
    s = np.broadcast_to(s, (x.shape[1],)) if s.size == 1 else s
    return x / np.sqrt((x * x).sum(axis=1, keepdims=True) + eps) * s[None, :, None, None]


def gather(heads):
    """Concat(axis 1) of Flatten(Permute(0, 2, 3, 1)(h)) over NCHW arrays h: (N, sum H W C)."""
    return np.concatenate([np.asarray(h).transpose(0, 2, 3, 1).reshape(h.shape[0], -1) for h in heads], axis=1)


def row_softmax(x):
    x = np.asarray(x, F64)
    e = np.exp(x - x.max(axis=-1, keepdims=True))
    return e / e.sum(axis=-1, keepdims=True)


def decode(loc, priors, code_type, variance_encoded):
    """loc (P, 4), priors (2, P * 4) -> (P, 4) corners, no clipping."""
    loc = np.asarray(loc, F64).reshape(-1, 4)
    pb = np.asarray(priors, F64)[0].reshape(-1, 4)
    v = np.ones_like(pb) if variance_encoded else np.asarray(priors, F64)[1].reshape(-1, 4)
    if code_type == CORNER:
        return pb + v * loc
    pw, ph = pb[:, 2] - pb[:, 0], pb[:, 3] - pb[:, 1]
    pcx, pcy = (pb[:, 0] + pb[:, 2]) / 2, (pb[:, 1] + pb[:, 3]) / 2
    cx, cy = v[:, 0] * loc[:, 0] * pw + pcx, v[:, 1] * loc[:, 1] * ph + pcy
    w, h = np.exp(v[:, 2] * loc[:, 2]) * pw, np.exp(v[:, 3] * loc[:, 3]) * ph
    return np.stack([cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2], axis=1)


def area(b):
    return 0.0 if b[2] < b[0] or b[3] < b[1] else (b[2] - b[0]) * (b[3] - b[1])


def jaccard(a, b):
    if b[0] > a[2] or b[2] < a[0] or b[1] > a[3] or b[3] < a[1]:
        return 0.0
    iw, ih = min(a[2], b[2]) - max(a[0], b[0]), min(a[3], b[3]) - max(a[1], b[1])
    if iw <= 0 or ih <= 0:
        return 0.0
    inter = iw * ih
    return inter / (area(a) + area(b) - inter)


def detection_output(loc, conf, priors, num_classes, background=0, nms_threshold=0.3, top_k=-1, code_type=CORNER, variance_encoded=False,
                     keep_top_k=-1, confidence_threshold=-np.inf):
    """loc (N, P * 4), conf (N, P * classes), priors (1, 2, P * 4) or (2, P * 4) -> (rows (K, 7) float64, margin).  With K == 0 the rows are
    Caffe's (N, 7) block of -1 with the image index in column 0, and `count` (third value) is 0."""
    loc, conf = np.asarray(loc, F64), np.asarray(conf, F64)
    priors = np.asarray(priors, F64).reshape(2, -1)
    n_img, p = loc.shape[0], loc.shape[1] // 4
    margin = np.inf
    rows = []
    for n in range(n_img):
        boxes = decode(loc[n], priors, code_type, variance_encoded)
        scores = conf[n].reshape(p, num_classes)
        survivors = []                                  # (score, label, prior), in row order
        for c in range(num_classes):
            if c == background:
                continue
            sc = scores[:, c]
            margin = min(margin, float(np.min(np.abs(sc - confidence_threshold)))) if np.isfinite(confidence_threshold) else margin
            cand = [i for i in range(p) if sc[i] > confidence_threshold]
            cand.sort(key=lambda i: (-sc[i], i))        # score descending, ties by prior index ascending (a stable sort's order)
            if top_k > -1 and len(cand) > top_k:
                if sc[cand[top_k - 1]] != sc[cand[top_k]]:
                    margin = min(margin, float(sc[cand[top_k - 1]] - sc[cand[top_k]]))
                cand = cand[:top_k]
            kept = []
            for i in cand:
                keep = True
                for j in kept:
                    ov = jaccard(boxes[i], boxes[j])
                    margin = min(margin, abs(ov - nms_threshold))
                    if ov > nms_threshold:
                        keep = False
                        break
                if keep:
                    kept.append(i)
            survivors += [(sc[i], c, i) for i in kept]
        if keep_top_k > -1 and len(survivors) > keep_top_k:
            order = sorted(range(len(survivors)), key=lambda q: (-survivors[q][0], survivors[q][1], survivors[q][2]))
            a, b = survivors[order[keep_top_k - 1]][0], survivors[order[keep_top_k]][0]
            if a != b:
                margin = min(margin, float(a - b))
            chosen = set(order[:keep_top_k])
            survivors = [s for q, s in enumerate(survivors) if q in chosen]
        rows += [[n, c, s] + list(boxes[i]) for s, c, i in survivors]
    if not rows:
        out = np.full((n_img, 7), -1.0, F64)
        out[:, 0] = np.arange(n_img)
        return out, margin, 0
    return np.array(rows, F64), margin, len(rows)
