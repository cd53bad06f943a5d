"""Guard-banded, bit-exact parity of fcn_detect_decode_group, fcn_gen_targets and fcn_gen_targets_nhwc (csrc/detect.hip), -m gpu.

Decode: the coverage and bbox maps are channel slices (cvg_cstride = C + 3 at offset 2, box_cstride = 4C + 5 at offset 3) of images whose
strides are 7 floats larger than an image; every pad, gap and red zone holds 3e38, not NaN: `NaN >= thresh` is false, so a consumed NaN
would be "no candidate" and show nothing, whereas 3e38 fires.  The workspace is exactly fcn_detect_workspace_bytes() of poison except its
last batch * num_classes words, the arrival words, which are zero as the header demands; it is NOT reset between the two launches of a case,
so the second launch meets arrival words that carry the first one's tag.  Outputs start as poison: entries at or beyond min(count, max_out)
of a slot must still be poison bit for bit.  The reference is the LITERAL cv::partition of oracle/detect_ref.py (fast=False) through
group_rectangles and the height filter of vote_boxes; tests/test_byte_refs.py cross-checks it against partition_fast and asserts that the
dense scene reaches every filter.  Targets: the NCHW outputs start as poison and must be written everywhere, zeros included; the NHWC form
writes channel slices of poisoned pixels and must hold the same values.  All comparisons are for equality."""
import ctypes as C

import numpy as np
import pytest

import byte_cases as B
from fcn_object_detector_amd import lib as L
from gpu_util import POISON_WORD, channels_untouched, g, launched_twice, poison_free, poisoned  # noqa: F401 (g: fixture)

pytestmark = pytest.mark.gpu
E_ARG, E_UNSUPPORTED = 1, 3
MODES = {"nearest_even": L.RECT_ROUND_NEAREST_EVEN, "trunc": L.RECT_ROUND_TRUNCATE}
GAP = 7


def det_params(c, gy, gx, mode="nearest_even", group_thresh=3, max_out=16):
    return L.DetectParams(c, gy, gx, B.DET_STRIDE, B.DET_STRIDE, c + 3, 2, 4 * c + 5, 3, B.DET_THRESH, group_thresh, B.DET_EPS, B.DET_MIN_HEIGHT,
                          MODES[mode], max_out)


def sliced_image(x, cstride, coffset):
    """(n, c, gy, gx) -> (n, gy * gx * cstride + GAP) floats: NHWC channel slice, every other float 3e38."""
    n, c, gy, gx = x.shape
    img = poisoned((n, gy * gx, cstride), "huge")
    img[..., coffset:coffset + c] = x.transpose(0, 2, 3, 1).reshape(n, gy * gx, c)
    flat = poisoned((n, gy * gx * cstride + GAP), "huge")
    flat[:, :gy * gx * cstride] = img.reshape(n, -1)
    return flat


def upload_maps(g, name):
    cvg, bb = B.detect_scene(name)
    c = cvg.shape[1]
    return (g.put(sliced_image(cvg, c + 3, 2), at_end=True, poison="huge", name="coverage"),
            g.put(sliced_image(bb, 4 * c + 5, 3), at_end=True, poison="huge", name="bbox"))


def workspace(g, p, batch, slices):
    """Exactly the documented size, poison except the arrival words (the last word of every problem), which are zero."""
    problems, cells = batch * p.num_classes, p.gy * p.gx
    nbytes = int(L.load().fcn_detect_workspace_bytes(C.byref(p), batch))
    assert nbytes == (problems * (5 + slices) * cells + problems) * 4, "this launch shape was meant to run %d workgroups per problem" % slices
    words = np.full(nbytes // 4, POISON_WORD, np.uint32)
    words[-problems:] = 0
    return g.put(words, name="workspace")


def expected_outputs(slots, max_out):
    rects, weights = poisoned((len(slots), max_out, 4), dtype=np.int32), poisoned((len(slots), max_out), dtype=np.int32)
    count = np.zeros(len(slots), np.int32)
    for s, (n, r, w) in enumerate(slots):
        count[s] = n
        k = max(min(n, max_out), 0)
        if k:
            rects[s, :k], weights[s, :k] = np.asarray(r[:k], np.int32), np.asarray(w[:k], np.int32)
    return rects, weights, count


def decode(g, name, slices, mode="nearest_even", group_thresh=3, max_out=16, ws=None, launches=2):
    cvg, bb = B.detect_scene(name)
    n, c, gy, gx = cvg.shape
    p = det_params(c, gy, gx, mode, group_thresh, max_out)
    d_cvg, d_box = upload_maps(g, name)
    ws = ws or workspace(g, p, n, slices)
    slots = n * c
    d_rects, d_weights, d_count = (g.put(slots * max_out * 16, name="out_rects"), g.put(slots * max_out * 4, name="out_weights"),
                                   g.put(slots * 4, at_end=True, name="out_count"))

    def call():
        L.call("fcn_detect_decode_group", d_cvg.ptr, d_box.ptr, n, gy * gx * (c + 3) + GAP, gy * gx * (4 * c + 5) + GAP, C.byref(p), ws.ptr,
               d_rects.ptr, d_weights.ptr, d_count.ptr, None)

    def read():
        return d_count.read((slots,), np.int32), d_rects.read((slots, max_out, 4), np.int32), d_weights.read((slots, max_out), np.int32)

    if launches == 2:
        got = launched_twice(call, read)
    else:
        call()
        got = read()
    assert d_cvg.unchanged() and d_box.unchanged(), "an input map was written"
    want_rects, want_weights, want_count = expected_outputs(B.detect_expected(name, mode, group_thresh), max_out)
    for what, a, b in zip(("count", "rects", "weights"), got, (want_count, want_rects, want_weights)):
        bad = np.nonzero((a != b).reshape(len(a), -1).any(axis=1))[0]
        assert a.tobytes() == b.tobytes(), "%s %s: slots %s differ, the first: got %s, expected %s" % (name, what, bad[:8], a[bad[:1]], b[bad[:1]])
    return ws


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("seed", B.DENSE_SEEDS)
def test_dense_scene_eight_workgroups_hand_over(g, seed, mode):
    """255 candidates > 192: the SimilarRects tests are dealt to eight workgroups and the last to arrive merges the forests."""
    decode(g, "dense%d" % seed, 8, mode)


@pytest.mark.parametrize("mode", list(MODES))
def test_few_candidates_one_workgroup_of_eight(g, mode):
    decode(g, "small", 8, mode)


@pytest.mark.parametrize("mode", list(MODES))
def test_fifty_problems_five_workgroups_each(g, mode):
    """One class of image 1 is dense; the others are sparse, empty, or a single all-zero box (the `.any()` exit)."""
    decode(g, "batch2", 5, mode, max_out=8)


def test_full_batch_one_workgroup_per_problem(g):
    decode(g, "batch43", 1, max_out=4)


@pytest.mark.parametrize("max_out", [96, 5])
def test_group_threshold_zero_passes_the_candidates_through(g, max_out):
    """More than 5 candidates pass the height filter: with max_out = 5 the count exceeds it, five are stored, and a sixth store would land
    behind the output arrays of this one-slot launch."""
    decode(g, "small", 8, group_thresh=0, max_out=max_out)


def test_more_survivors_than_max_out(g):
    """count 3, two stored.  Slot 0's third store would land in slot 1, whose class has no candidate: nobody writes there, and it must still
    be poison; slot 2 is the last one, so its third store would land in the red zone behind the output arrays."""
    assert [s[0] for s in B.detect_expected("three")] == [3, 0, 3]
    decode(g, "three", 8, max_out=2)


def test_more_candidates_than_the_kernel_holds(g):
    """5184 candidates: that slot's count is -1 and its rects and weights remain poison; the class next to it is decoded normally."""
    decode(g, "overflow", 8)


def test_one_workspace_serves_launch_after_launch(g):
    """Never reset: each launch meets the arrival words, forests and lists of the one before, left by another scene and rounding mode."""
    ws = decode(g, "dense0", 8, "nearest_even", launches=1)
    decode(g, "dense1", 8, "trunc", ws=ws, launches=1)
    decode(g, "dense0", 8, "trunc", ws=ws)


def test_decode_refusals_leave_the_buffers_alone(g):
    cvg, bb = B.detect_scene("small")
    d_cvg, d_box = upload_maps(g, "small")
    good = det_params(1, 9, 10)
    ws = workspace(g, good, 1, 8)
    outs = [g.put(16 * 16, name="out_rects"), g.put(16 * 4, name="out_weights"), g.put(16, name="out_count")]
    lib = L.load()

    def call(cv=d_cvg.ptr, bx=d_box.ptr, batch=1, p=good, w=ws.ptr, r=outs[0].ptr, wt=outs[1].ptr, ct=outs[2].ptr):
        return lib.fcn_detect_decode_group(cv, bx, batch, 90 * 4 + GAP, 90 * 9 + GAP, C.byref(p) if p is not None else None, w, r, wt, ct, None)

    def bad(**kw):
        p = det_params(1, 9, 10)
        for k, v in kw.items():
            setattr(p, k, v)
        return call(p=p)

    refused = [call(cv=None), call(bx=None), call(p=None), call(w=None), call(r=None), call(wt=None), call(ct=None), call(batch=0),      # null / empty
               bad(num_classes=0), bad(gy=0), bad(gx=-1), bad(max_out=0),                                                                  # extents
               bad(cvg_coffset=-1), bad(cvg_cstride=2), bad(box_coffset=-1), bad(box_cstride=6), bad(round_mode=2)]                      # slices, mode
    assert all(rc == E_ARG for rc in refused), refused
    assert bad(gy=4096, gx=4096) == E_UNSUPPORTED and call(batch=1 << 30) == E_UNSUPPORTED                                               # too large
    L.call("fcn_device_sync")
    assert d_cvg.unchanged() and d_box.unchanged() and ws.unchanged() and all(o.unchanged() for o in outs)


# ---------------------------------------------------------------------------------------------------------------- targets
def upload_targets(g):
    t = B.TGT
    rects = np.asarray([r for rs in t["rects"] for r in rs], np.int32).reshape(-1, 4)
    labels = np.asarray([l for ls in t["labels"] for l in ls], np.int32)
    offs = np.cumsum([0] + [len(rs) for rs in t["rects"]]).astype(np.int32)
    assert offs[0] == offs[1] and offs[-1] == len(rects) == len(labels)          # image 0 has no boxes: its two offsets are equal
    return [g.put(a, at_end=True, name=n) for a, n in ((rects, "rects"), (labels, "labels"), (offs, "rect_offsets"))]


def test_gen_targets_nchw_and_nhwc(g):
    t = B.TGT
    n, c, gy, gx = t["batch"], t["C"], t["gy"], t["gx"]
    want = B.targets_expected()
    ins = upload_targets(g)
    geom = (n, c, gy, gx, t["stride"], t["iou"])
    outs = [g.put(poisoned(w.shape), at_end=True, name="nchw %d" % k) for k, w in enumerate(want)]
    got = []
    for _ in range(2):
        L.call("fcn_gen_targets", *(b.ptr for b in ins), *geom, *(o.ptr for o in outs), None)
        L.call("fcn_device_sync")
        got.append([o.read(w.shape) for o, w in zip(outs, want)])
    names = ("foreground", "bbox", "size", "obj", "coverage")
    for k, name in enumerate(names):
        assert got[0][k].tobytes() == got[1][k].tobytes(), "two launches differ"
        assert poison_free(got[0][k]), "%s: an element was not written" % name
        assert got[0][k].tobytes() == want[k].tobytes(), "%s: %d elements differ" % (name, int((got[0][k] != want[k]).sum()))
    fg_cs, blk_cs = c + 2, 4 * c + 3
    nhwc = [g.put(poisoned((n, gy, gx, fg_cs if k == 0 else blk_cs)), at_end=True, name="nhwc %d" % k) for k in range(5)]
    full = []
    for _ in range(2):
        L.call("fcn_gen_targets_nhwc", *(b.ptr for b in ins), *geom, nhwc[0].ptr, fg_cs, *(o.ptr for o in nhwc[1:]), blk_cs, None)
        L.call("fcn_device_sync")
        full.append([o.read((n, gy, gx, fg_cs if k == 0 else blk_cs)) for k, o in enumerate(nhwc)])
    for k, name in enumerate(names):
        ch = c if k == 0 else 4 * c
        a = full[0][k]
        assert a.tobytes() == full[1][k].tobytes(), "two launches differ"
        assert channels_untouched(a, np.arange(a.shape[-1]) < ch), "%s: a pad channel was written" % name
        vals = np.ascontiguousarray(a[..., :ch].transpose(0, 3, 1, 2))
        assert vals.tobytes() == want[k].tobytes() == got[0][k].tobytes(), "%s: the two layouts differ" % name
    assert all(b.unchanged() for b in ins)


def test_gen_targets_refusals_leave_the_buffers_alone(g):
    t = B.TGT
    n, c, gy, gx = t["batch"], t["C"], t["gy"], t["gx"]
    ins = upload_targets(g)
    outs = [g.put(poisoned((n, gy, gx, c + 2 if k == 0 else 4 * c + 3)), name="out %d" % k) for k in range(5)]
    lib = L.load()

    def nchw(i=None, o=None, geom=(n, c, gy, gx, t["stride"])):
        ip, op = [b.ptr for b in ins], [b.ptr for b in outs]
        if i is not None:
            ip[i] = None
        if o is not None:
            op[o] = None
        return lib.fcn_gen_targets(*ip, *geom, t["iou"], *op, None)

    def nhwc(i=None, o=None, geom=(n, c, gy, gx, t["stride"]), fg_cs=c + 2, blk_cs=4 * c + 3):
        ip, op = [b.ptr for b in ins], [b.ptr for b in outs]
        if i is not None:
            ip[i] = None
        if o is not None:
            op[o] = None
        return lib.fcn_gen_targets_nhwc(*ip, *geom, t["iou"], op[0], fg_cs, *op[1:], blk_cs, None)

    extents = [(0, c, gy, gx, 8), (n, 0, gy, gx, 8), (n, c, 0, gx, 8), (n, c, gy, -1, 8), (n, c, gy, gx, 0)]
    refused = ([f(i=k) for f in (nchw, nhwc) for k in range(3)] + [f(o=k) for f in (nchw, nhwc) for k in range(5)]
               + [f(geom=e) for f in (nchw, nhwc) for e in extents] + [nhwc(fg_cs=c - 1), nhwc(blk_cs=4 * c - 1)])
    assert all(rc == E_ARG for rc in refused), refused
    L.call("fcn_device_sync")
    assert all(b.unchanged() for b in ins + outs)
