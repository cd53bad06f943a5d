"""Guard-banded, bit-exact parity of the scene renderer and the label resize (csrc/scene.hip), -m gpu.

The background (11 x 13), the object images and masks (6 x 7) and the fcn_scene_obj records end on the last byte in front of their back
red zones (256 KiB of poison on either side) and must be bit-identical after the launch; byte outputs start as the bitwise complement of
the expected result, so a byte the kernel never wrote cannot pass; every case is launched twice on the same buffers.  The reference is
oracle/scene_ref.py::render_scene driven with a stand-in layer and hand-written plans (tests/byte_cases.py); the permutation-only scenes
- background crop of the scene's size, objects with out == roi: no arithmetic happens - are held to an image built by slicing alone
(tests/ref_bytes.py).  fcn_mask_to_label_f32 writes one channel of poisoned pixels.  All comparisons are for equality."""
import ctypes as C

import numpy as np
import pytest

import byte_cases as B
import ref_bytes as RB
from fcn_object_detector_amd import lib as L
from gpu_util import complement, g, launched_twice, poisoned, slice_untouched  # noqa: F401 (g: fixture)

pytestmark = pytest.mark.gpu
E_ARG = 1
CASES = B.compose_cases()


def upload_scene(g, objects):
    """-> (background, [(image, mask) buffers], record buffer or None): every input at the end of its allocation."""
    bg = g.put(B.BACKGROUND, at_end=True, name="background")
    srcs = [(g.put(i, at_end=True, name="object image %d" % k), g.put(m, at_end=True, name="object mask %d" % k)) for k, (i, m) in enumerate(B.SOURCES)]
    recs = (L.SceneObj * max(len(objects), 1))()
    for r, o in zip(recs, objects):
        r.img, r.mask = srcs[o["idx"]][0].ptr, srcs[o["idx"]][1].ptr
        r.src_h, r.src_w, r.flip = B.SRC_H, B.SRC_W, o["flip"]
        r.roi_x, r.roi_y, r.roi_w, r.roi_h = o["roi"]
        r.out_w, r.out_h = o["out"]
        r.cx, r.cy = o["pos"]
        r.label1 = o["label"] + 1
    assert C.sizeof(L.SceneObj) == 64
    objs = g.put(np.frombuffer(bytes(recs), np.uint8)[:64 * len(objects)].copy(), at_end=True, name="records") if objects else None
    return bg, srcs, objs


def inputs_unchanged(bg, srcs, objs):
    return bg.unchanged() and all(i.unchanged() and m.unchanged() for i, m in srcs) and (objs is None or objs.unchanged())


@pytest.mark.parametrize("name", list(CASES))
def test_compose(g, name):
    p, outs, entry, perm = CASES[name]
    want_img, want_mask = B.compose_expected(p)
    vx, vy, vw, vh = p["view"] or (0, 0, B.SCENE_W, B.SCENE_H)
    if perm:
        img, mask = RB.compose_permutation(B.BACKGROUND, p["bg_crop"][:2], B.SCENE_H, B.SCENE_W, B.SOURCES, p["objects"], p["final_flip"])
        assert np.array_equal(img[vy:vy + vh, vx:vx + vw], want_img) and np.array_equal(mask[vy:vy + vh, vx:vx + vw], want_mask)
    assert want_img.shape == (vh, vw, 3) and want_mask.shape == (vh, vw)
    bg, srcs, objs = upload_scene(g, p["objects"])
    d_img = g.put(complement(want_img), at_end=True, name="out_img") if outs != "mask" else None
    d_mask = g.put(complement(want_mask), at_end=True, name="out_mask") if outs != "img" else None
    args = (bg.ptr, B.BG_H, B.BG_W, *p["bg_crop"], objs.ptr if objs else None, len(p["objects"]), p["final_flip"],
            d_img.ptr if d_img else None, d_mask.ptr if d_mask else None, B.SCENE_H, B.SCENE_W)
    if entry == "plain":
        call = lambda: L.call("fcn_compose_scene_bgr8", *args, None)
    else:
        call = lambda: L.call("fcn_compose_scene_view_bgr8", *args, vx, vy, vw, vh, None)
    got = launched_twice(call, lambda: [d.read(w.shape, np.uint8) for d, w in ((d_img, want_img), (d_mask, want_mask)) if d is not None])
    assert inputs_unchanged(bg, srcs, objs)
    if d_img:
        assert got[0].tobytes() == want_img.tobytes(), "%s: %d image bytes differ" % (name, int((got[0] != want_img).sum()))
    if d_mask:
        assert got[-1].tobytes() == want_mask.tobytes(), "%s: %d mask bytes differ" % (name, int((got[-1] != want_mask).sum()))


def test_compose_refusals_leave_the_buffers_alone(g):
    bg, srcs, objs = upload_scene(g, B.OBJECTS)
    d_img, d_mask = g.put(B.SCENE_H * B.SCENE_W * 3, name="out_img"), g.put(B.SCENE_H * B.SCENE_W, name="out_mask")
    lib = L.load()
    H, W, n = B.SCENE_H, B.SCENE_W, len(B.OBJECTS)

    def view(bgp=bg.ptr, bg_hw=(B.BG_H, B.BG_W), crop=B.MAIN_CROP, o=objs.ptr, nobj=n, im=d_img.ptr, mk=d_mask.ptr, hw=(H, W), v=(0, 0, W, H)):
        return lib.fcn_compose_scene_view_bgr8(bgp, *bg_hw, *crop, o, nobj, 0, im, mk, *hw, *v, None)

    refused = [view(bgp=None), view(im=None, mk=None), view(o=None), view(nobj=-1), view(bg_hw=(0, B.BG_W)), view(hw=(0, W)),       # null, extents
               view(v=(-1, 0, 4, 4)), view(v=(0, 0, W + 1, H)), view(v=(8, 7, 5, 4)), view(v=(0, 0, 0, 4)),                             # view outside
               view(crop=(-1, 0, 4, 4)), view(crop=(5, 0, 9, 7)), view(crop=(0, 5, 9, 7)), view(crop=(0, 0, 0, 7)),                     # crop outside
               lib.fcn_compose_scene_bgr8(bg.ptr, B.BG_H, B.BG_W, *B.MAIN_CROP, objs.ptr, n, 0, None, d_mask.ptr, H, W, None),           # no image
               lib.fcn_compose_scene_bgr8(None, B.BG_H, B.BG_W, *B.MAIN_CROP, objs.ptr, n, 0, d_img.ptr, d_mask.ptr, H, W, None)]
    assert all(rc == E_ARG for rc in refused), refused
    assert view(hw=(1 << 15, 1 << 15), v=(0, 0, 4, 4)) != 0                                                                               # scene too large
    L.call("fcn_device_sync")
    assert inputs_unchanged(bg, srcs, objs) and d_img.unchanged() and d_mask.unchanged()


@pytest.mark.parametrize("cstride", [1, 3])
@pytest.mark.parametrize("hw", B.LABEL_SIZES, ids=str)
def test_mask_to_label(g, hw, cstride):
    """One float per pixel at stride dst_cstride; with 3, the label is channel 1 of poisoned pixels and channels 0 and 2 stay poison."""
    H, W = hw
    want = B.label_expected(hw)
    if hw == (14, 18):
        assert want.tobytes() == RB.label_repeat(B.LABEL_MASK, 2, 2).tobytes()
    off = 1 if cstride == 3 else 0
    mask = g.put(B.LABEL_MASK, at_end=True, name="mask")
    dst = g.put(poisoned((H, W, cstride)), at_end=(cstride == 1), name="dst")
    full = launched_twice(lambda: L.call("fcn_mask_to_label_f32", mask.ptr, 7, 9, dst.ptr + 4 * off, H, W, cstride, None),
                     lambda: dst.read((H, W, cstride)))
    assert mask.unchanged() and slice_untouched(full, off, 1)
    assert full[..., off].tobytes() == want.tobytes(), "%d labels differ" % int((full[..., off] != want).sum())


def test_mask_to_label_refusals(g):
    mask, dst = g.put(B.LABEL_MASK, at_end=True, name="mask"), g.put(poisoned((7, 9, 1)), name="dst")
    lib = L.load()
    refused = [lib.fcn_mask_to_label_f32(None, 7, 9, dst.ptr, 7, 9, 1, None), lib.fcn_mask_to_label_f32(mask.ptr, 7, 9, None, 7, 9, 1, None),
               lib.fcn_mask_to_label_f32(mask.ptr, 0, 9, dst.ptr, 7, 9, 1, None), lib.fcn_mask_to_label_f32(mask.ptr, 7, 9, dst.ptr, 7, 0, 1, None),
               lib.fcn_mask_to_label_f32(mask.ptr, 7, 9, dst.ptr, 7, 9, 0, None)]
    assert all(rc == E_ARG for rc in refused), refused
    L.call("fcn_device_sync")
    assert mask.unchanged() and dst.unchanged()
