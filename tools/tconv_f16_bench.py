#!/usr/bin/env python3
"""Times the half-float transposed convolution (fcn_tconv2d_f16, csrc/tconv.hip) under each of its tile configurations beside the
float32 kernel (fcn_tconv2d_f32) on the same shapes, each kernel alone on the GPU, and `caffe time` of FCN-8s in both engines (not
imported by the package).

Layers, at the sizes a 500 x 500 image gives the published nets with 21 classes (pad 100: pool5 is 22 x 22, score_fr 16 x 16), batch 1:

  upscore        FCN-32s  k64 s32  21 -> 21   16 x 16  -> 544 x 544
  upscore16      FCN-16s  k32 s16  21 -> 21   34 x 34  -> 560 x 560
  upscore8       FCN-8s   k16 s8   21 -> 21   70 x 70  -> 568 x 568
  upscore2       FCN-16s  k4 s2    21 -> 21   16 x 16  -> 34 x 34
  decoder k2s2   a DeconvNet / U-Net step  k2 s2  256 -> 128  64 x 64 -> 128 x 128

`--runs` windows of `--reps` launches back to back, the kernels taking turns window by window: the median and the range of the
per-launch time and the ratio half / float32.  Beside every half launch its distance to its own two floors:

  stores   the bytes of the result at 6.3 TB/s (what a float4 copy reaches on this chip);
  mfma     the padded matrix work: tiles x taps x 32-channel chunks of every phase, two v_mfma_f32_32x32x16_f16 per wave and chunk at 32
           cycles each, four waves per workgroup, over 256 CUs x 4 SIMDs at 2.4 GHz.

    python tools/tconv_f16_bench.py [--runs 7] [--reps 100] [--net-iterations 20] [--no-net]
"""
import argparse
import ctypes as C
import os
import re
import statistics
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from fcn_object_detector_amd import lib as L  # noqa: E402
from fcn_object_detector_amd import models  # noqa: E402
from fcn_object_detector_amd.engine import DeviceBuffer  # noqa: E402

# name, Ca, Cb, k, s, H = W
LAYERS = [("upscore", 21, 21, 64, 32, 16), ("upscore16", 21, 21, 32, 16, 34), ("upscore8", 21, 21, 16, 8, 70), ("upscore2", 21, 21, 4, 2, 16),
          ("decoder k2s2", 256, 128, 2, 2, 64)]
HBM, CLOCK, SIMDS, MFMA_CYCLES = 6.3e12, 2.4e9, 256 * 4, 32
TILES = {0: (64, 64), 1: (128, 32)}


def r8(c):
    return (c + 7) // 8 * 8


def mfma_floor_us(ca, cb, k, s, h, bm, bn):
    """The padded matrix work of one launch: every phase's tiles x taps x chunks, 2 MFMAs per wave and chunk, 4 waves per workgroup."""
    oh = s * (h - 1) + k
    chunks = (r8(ca) + 31) // 32
    mfmas = 0
    for f in range(s):
        for g in range(s):
            ly, lx = (oh - 1 - f) // s + 1, (oh - 1 - g) // s + 1
            ty, tx = (k - f + s - 1) // s, (k - g + s - 1) // s
            mfmas += -(-ly * lx // bm) * -(-cb // bn) * ty * tx * chunks * 2 * 4
    return mfmas * MFMA_CYCLES / SIMDS / CLOCK * 1e6


def caffe_time(path, dtype, iterations):
    env = dict(os.environ, FCN_DTYPE=dtype)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "fcn_object_detector_amd", "caffe_tool.py"), "time", "--model=" + path,
                          "--iterations=%d" % iterations], env=env, capture_output=True, text=True, check=True).stderr
    rows = {m.group(1): float(m.group(2)) for m in re.finditer(r"^\s*(\S+)\tforward: (\S+) ms", out, flags=re.M)}
    return float(re.search(r"Average Forward pass: (\S+) ms", out).group(1)), rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--net-iterations", type=int, default=20)
    ap.add_argument("--no-net", action="store_true")
    a = ap.parse_args()
    lib = L.load()
    L.call("fcn_init", 0)
    sp = C.c_void_p()
    L.call("fcn_stream_create", C.byref(sp))
    st = sp.value
    e0, e1 = C.c_void_p(), C.c_void_p()
    L.call("fcn_event_create", C.byref(e0))
    L.call("fcn_event_create", C.byref(e1))

    def window(fn):
        L.call("fcn_event_record", e0, st)
        for _ in range(a.reps):
            fn()
        L.call("fcn_event_record", e1, st)
        L.call("fcn_event_sync", e1)
        ms = C.c_float()
        L.call("fcn_event_elapsed_ms", e0, e1, C.byref(ms))
        return 1e3 * ms.value / a.reps

    def upload(arr):
        arr = np.ascontiguousarray(arr)
        buf = DeviceBuffer(arr.nbytes, zero=False)
        L.call("fcn_memcpy_h2d_async", buf.ptr, arr.ctypes.data, arr.nbytes, st)
        L.call("fcn_stream_sync", st)
        return buf

    ncfg = int(lib.fcn_tconv2d_num_configs_f16())
    print("%d windows of %d launches each, the kernels taking turns: median (min .. max) us per launch; floors in us" % (a.runs, a.reps))
    rng = np.random.default_rng(0)
    for name, ca, cb, k, s, h in LAYERS:
        oh = s * (h - 1) + k
        x = rng.standard_normal((1, h, h, ca)).astype(np.float32)
        w = (rng.standard_normal((k, k, cb, ca)) / np.sqrt(ca)).astype(np.float32)      # the packed bank [kh][kw][Cb][Ca]
        b = upload(rng.standard_normal(cb).astype(np.float32))
        keep, fns = [b], {}
        for key, dt, vec, prepare, launch, cfg in [("f32", np.float32, 4, "fcn_tconv2d_prepare", lib.fcn_tconv2d_f32, -1)] + [
                ("f16 cfg%d" % c, np.float16, 8, "fcn_tconv2d_prepare_f16", lib.fcn_tconv2d_f16, c) for c in range(ncfg)]:
            cap, cbp = (ca + vec - 1) // vec * vec, (cb + vec - 1) // vec * vec
            xp, wp = np.zeros((1, h, h, cap), dt), np.zeros((k, k, cb, cap), dt)
            xp[..., :ca], wp[..., :ca] = x, w
            xb, wb = upload(xp), upload(wp)
            yb = DeviceBuffer(np.dtype(dt).itemsize * oh * oh * cbp)
            d = L.TConvDesc()
            d.a, d.w, d.bias, d.b = xb.ptr, wb.ptr, b.ptr, yb.ptr
            d.N, d.H, d.W, d.Ca, d.a_cstride = 1, h, h, ca, cap
            d.Cb, d.kh, d.kw, d.pad, d.stride, d.OH, d.OW = cb, k, k, 0, s, oh, oh
            d.b_cstride, d.b_coffset, d.flags = cbp, 0, 0
            ws = DeviceBuffer(int(lib.fcn_tconv2d_workspace_bytes(C.byref(d), 1)), zero=False)
            plan = L.TConvPlan()
            L.call(prepare, C.byref(d), 1, ws.ptr, cfg, C.byref(plan))
            keep.extend([xb, wb, yb, d, ws, plan])
            fns[key] = lambda plan=plan, launch=launch: L.check(launch(C.byref(plan), st))
        us = {key: [] for key in fns}
        for fn in fns.values():      # warm up all
            fn()
        L.call("fcn_stream_sync", st)
        for _ in range(a.runs):
            for key, fn in fns.items():
                us[key].append(window(fn))
        med = {key: statistics.median(v) for key, v in us.items()}
        store16 = 2.0 * oh * oh * cb / HBM * 1e6
        print("%-13s k%-2d s%-2d %3d->%-3d %3d -> %3d  f32 %7.1f (%.1f .. %.1f)" % (name, k, s, ca, cb, h, oh, med["f32"], min(us["f32"]), max(us["f32"])),
              end="")
        for c in range(ncfg):
            key = "f16 cfg%d" % c
            mf = mfma_floor_us(ca, cb, k, s, h, *TILES[c])
            print(" | cfg%d %7.1f (%.1f .. %.1f) x%.2f, stores %.1f (x%.1f), mfma %.1f (x%.1f)" % (
                c, med[key], min(us[key]), max(us[key]), med[key] / med["f32"], store16, med[key] / store16, mf, med[key] / mf), end="")
        print(flush=True)
        for buf in keep:
            if isinstance(buf, DeviceBuffer):
                buf.free()
    if a.no_net:
        return
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "fcn8s.prototxt")
        open(path, "w").write(models.voc_fcn8s("TEST", fillers=True))
        for dtype in ("f32", "f16"):
            ms, rows = caffe_time(path, dtype, a.net_iterations)
            tail = " ".join("%s %.3f" % (n, rows[n]) for n in ("upscore2", "upscore_pool4", "upscore8", "score") if n in rows)
            print("caffe time FCN-8s 500 x 500 %s: %.3f ms per forward; ms per op: %s" % (dtype, ms, tail), flush=True)


if __name__ == "__main__":
    main()
