"""Independent references of the byte and integer kernels: plain numpy / scipy, nothing from the package under test and nothing from
oracle/.  tests/test_byte_refs.py holds them to the oracle on the inputs of tests/byte_cases.py; the guarded GPU tests compare the
kernels with both."""
import numpy as np
from scipy import ndimage as ndi


def blur_box(img: np.ndarray, k: int) -> np.ndarray:
    """cv2.blur(img, (k, k)): scipy's 'mirror' is reflect-101 and its window of an even k starts at x - k // 2, the anchor k / 2."""
    out = np.empty_like(img)
    for c in range(img.shape[2]):
        total = ndi.correlate(img[..., c].astype(np.int64), np.ones((k, k), np.int64), mode="mirror")
        out[..., c] = np.rint(total * (1.0 / (k * k)))
    return out


def blur_median(img: np.ndarray, k: int) -> np.ndarray:
    """cv2.medianBlur(img, k), k odd: per-channel median, replicated border."""
    return np.stack([ndi.median_filter(img[..., c], size=k, mode="nearest") for c in range(img.shape[2])], axis=2)


def flip(a: np.ndarray, code: int) -> np.ndarray:
    """cv.flip codes 0 (rows), 1 (columns), -1 (both); anything else: none.  Slicing only."""
    if code == 0:
        return a[::-1]
    if code == 1:
        return a[:, ::-1]
    if code == -1:
        return a[::-1, ::-1]
    return a


def compose_permutation(bg, crop_xy, H, W, sources, objects, final_flip):
    """A scene in which no arithmetic happens - the background crop has the scene's size, every object has out == roi and a mask of
    zeros and one nonzero value - built by slicing and [::-1] alone.  objects: dicts idx, flip, roi (x, y, w, h), pos (cx, cy), label."""
    bx, by = crop_xy
    img = bg[by:by + H, bx:bx + W].copy()
    mask = np.zeros((H, W), np.uint8)
    for o in objects:
        simg, smsk = sources[o["idx"]]
        x, y, w, h = o["roi"]
        roi_i, roi_m = flip(simg, o["flip"])[y:y + h, x:x + w], flip(smsk, o["flip"])[y:y + h, x:x + w]
        cx, cy = o["pos"]
        x0, y0, x1, y1 = max(cx, 0), max(cy, 0), min(cx + w, W), min(cy + h, H)
        sel = roi_m[y0 - cy:y1 - cy, x0 - cx:x1 - cx] != 0
        img[y0:y1, x0:x1][sel] = roi_i[y0 - cy:y1 - cy, x0 - cx:x1 - cx][sel]
        mask[y0:y1, x0:x1][sel] = o["label"] + 1
    return flip(img, final_flip).copy(), flip(mask, final_flip).copy()


def label_repeat(mask: np.ndarray, fy: int, fx: int) -> np.ndarray:
    """Nearest-neighbour enlargement by whole factors."""
    return np.repeat(np.repeat(mask, fy, axis=0), fx, axis=1).astype(np.float32)


def rectangles_mask(shape, blocks):
    """blocks: (row0, col0, rows, cols, byte value) -> uint8 mask of disjoint filled rectangles."""
    m = np.zeros(shape, np.uint8)
    for r0, c0, nr, nc, v in blocks:
        assert not m[max(r0 - 1, 0):r0 + nr + 1, max(c0 - 1, 0):c0 + nc + 1].any(), "blocks must not touch (8-connectivity)"
        m[r0:r0 + nr, c0:c0 + nc] = v
    return m


def largest_rectangle(blocks):
    """(found, x, y, w, h) of disjoint filled rectangles: the outer border polygon of a w x h block runs through the pixel centres and
    has area (w - 1)(h - 1); the largest positive area wins, among equals the block whose first pixel comes LAST in raster order."""
    best = None
    for r0, c0, nr, nc, _v in blocks:
        area = (nc - 1) * (nr - 1)
        if area > 0 and (best is None or (area, r0, c0) >= best[0]):
            best = ((area, r0, c0), (1, c0, r0, nc, nr))
    return best[1] if best else (0, 0, 0, 0, 0)
