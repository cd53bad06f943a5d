"""Guard-banded, bit-exact parity of fcn_score_masks (csrc/mask.hip), -m gpu.

The score blob is one channel slice (coffset 1 of 5-channel pixels) placed at the end of its allocation.  Its pad channels, its red zones
AND its background class are poisoned with 3e38, not NaN: `v < thresh ? 0 : v` keeps a NaN, the clamp-and-cast then yields byte 0, so a
consumed NaN would read as background and show nothing, whereas 3e38 yields 2147483520 & 0xFF = 128: foreground in pmap and in the boxes.
The workspace is exactly fcn_score_masks_workspace_bytes() of poison (the header does not ask for a zeroed one), `out` is poison and every
one of its 5 * maps words must be written, pmap is zero-filled and sits in front of poison: its size (130 or 221 bytes) is no multiple of
4, and the bytes behind it, which the kernel's 32-bit OR reads and writes back unchanged, must be bit-identical afterwards.  Every case is
launched twice without re-zeroing pmap (OR is idempotent).  References: oracle/mask_ref.py::run_detector2_post without its padding and
the window origin, and analytic masks of disjoint filled rectangles that need no oracle (tests/byte_cases.py, tests/ref_bytes.py).
All comparisons are for equality."""
import numpy as np
import pytest

import byte_cases as B
from fcn_object_detector_amd import lib as L
from gpu_util import g, launched_twice, poisoned, poisoned_nhwc  # noqa: F401 (g: fixture)

pytestmark = pytest.mark.gpu
E_ARG, E_ALIGN = 1, 2
CSTRIDE, COFFSET = 5, 1


def device_scores(g, fm):
    """Classes 1 .. C-1 at channels COFFSET + 1 ..; channel COFFSET (the background class) and the pads hold 3e38."""
    c = fm.shape[1]
    assert CSTRIDE >= COFFSET + c
    return g.put(poisoned_nhwc(fm[:, 1:], CSTRIDE, COFFSET + 1, poison="huge"), at_end=True, poison="huge", name="score")


def run_score_masks(g, fm, rects, frame_hw, thresh=B.SCORE_THRESH):
    n, c, H, W = fm.shape
    w, h = rects[0][2:]
    maps = n * (c - 1)
    score = device_scores(g, fm)
    h_rects = np.asarray(rects, np.int32)
    ws_bytes = int(L.load().fcn_score_masks_workspace_bytes(n, c, w, h))
    assert ws_bytes >= maps * w * h * 5 + maps * 8
    ws = g.put(ws_bytes, name="workspace")
    pmap = g.put(np.zeros(frame_hw, np.uint8), name="pmap")
    out = g.put(poisoned((maps, 5), dtype=np.int32), at_end=True, name="out")
    got = launched_twice(lambda: L.call("fcn_score_masks", score.ptr, n, c, H, W, CSTRIDE, COFFSET, h_rects.ctypes.data, float(np.float32(thresh)),
                                        pmap.ptr, frame_hw[0], frame_hw[1], ws.ptr, out.ptr, None),
                         lambda: (pmap.read(frame_hw, np.uint8), out.read((maps, 5), np.int32)))
    assert score.unchanged(), "the score blob was written"
    return got


@pytest.mark.parametrize("win", B.SCORE_WINDOWS, ids=str)
def test_score_masks_match_the_oracle(g, win):
    fm, rects = B.score_case(win)
    want_pmap, want_out = B.score_expected(fm, rects, B.SCORE_FRAME)
    pmap, out = run_score_masks(g, fm, rects, B.SCORE_FRAME)
    assert pmap.tobytes() == want_pmap.tobytes(), "%d pmap bytes differ" % int((pmap != want_pmap).sum())
    assert out.tobytes() == want_out.tobytes(), (out.tolist(), want_out.tolist())


def test_analytic_rectangle_masks(g):
    """The largest outer border polygon wins ((w - 1)(h - 1) of a w x h block), among equals the block found last in raster order; a lone
    pixel and a one-pixel line have area 0 and are never selected; 1.5 wraps to 126; an empty class is five zeros."""
    fm, _ = B.analytic_scores()
    want_pmap, want_out = B.analytic_expected()
    pmap, out = run_score_masks(g, fm, B.ANALYTIC_RECTS, B.ANALYTIC_FRAME)
    assert out.tolist() == want_out.tolist() == [[1, 8, 6, 6, 3], [1, 9, 5, 3, 4], [0] * 5, [0] * 5]
    assert pmap.tobytes() == want_pmap.tobytes(), "%d pmap bytes differ" % int((pmap != want_pmap).sum())


def test_thirty_two_windows_are_accepted(g):
    fm, rects = B.many_windows(32)
    want_pmap, want_out = B.score_expected(fm, rects, B.SCORE_FRAME)
    pmap, out = run_score_masks(g, fm, rects, B.SCORE_FRAME)
    assert pmap.tobytes() == want_pmap.tobytes() and out.tobytes() == want_out.tobytes()


def test_refusals_leave_the_buffers_alone(g):
    fm, rects = B.many_windows(33)
    n, c, H, W = 2, 2, 2, 2
    score = device_scores(g, fm)
    ws = g.put(int(L.load().fcn_score_masks_workspace_bytes(33, 2, 2, 2)), name="workspace")
    pmap = g.put(np.zeros(B.SCORE_FRAME, np.uint8), name="pmap")
    out = g.put(poisoned((33, 5), dtype=np.int32), name="out")
    fh, fw = B.SCORE_FRAME
    lib = L.load()
    ok = np.asarray(rects, np.int32)
    unequal = ok.copy()
    unequal[1, 2] = 3
    empty = ok.copy()
    empty[:, 3] = 0

    def call(sc=score.ptr, n=n, c=c, H=H, W=W, cs=CSTRIDE, co=COFFSET, r=ok, pm=pmap.ptr, fh=fh, fw=fw, w=ws.ptr, o=out.ptr):
        return lib.fcn_score_masks(sc, n, c, H, W, cs, co, r.ctypes.data if r is not None else None, 0.5, pm, fh, fw, w, o, None)

    refused = [call(sc=None), call(r=None), call(pm=None), call(w=None), call(o=None),                                      # null
               call(n=0), call(n=33), call(c=1), call(H=0), call(W=0), call(cs=2), call(co=-1), call(co=4), call(fh=0), call(fw=0),      # extents
               call(r=unequal), call(r=empty)]                                                                                # windows
    assert all(rc == E_ARG for rc in refused), refused
    assert call(pm=pmap.ptr + 1) == E_ALIGN and call(pm=pmap.ptr + 2) == E_ALIGN
    L.call("fcn_device_sync")
    assert score.unchanged() and ws.unchanged() and pmap.unchanged() and out.unchanged()
