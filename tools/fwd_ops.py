#!/usr/bin/env python
"""GPU: per-launch HIP-event times of one forward of a deploy net.  usage: python tools/fwd_ops.py batch f32|f16 [builder]
builder: googlenet_detectnet_deploy (default), caffenet, goturn_tracker, bvlc_googlenet or resnet50 / resnet101 / resnet152 (their DEPLOY form)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from fcn_object_detector_amd import models, proto  # noqa: E402
from fcn_object_detector_amd.engine import Engine  # noqa: E402
from fcn_object_detector_amd.netspec import NetSpec, fill_params  # noqa: E402


def main():
    n, dtype = int(sys.argv[1]), sys.argv[2]
    builder = sys.argv[3] if len(sys.argv) > 3 else "googlenet_detectnet_deploy"
    fn = getattr(models, builder)
    msg = proto.parse_text(fn(batch=n) if builder == "googlenet_detectnet_deploy" else fn("DEPLOY", batch=n))
    spec = NetSpec(msg, "TEST")
    spec.infer()
    eng = Engine(NetSpec(msg, "TEST"), params=fill_params(spec, seed=1234), device=0, dtype=dtype)
    rng = np.random.default_rng(0)
    for nm in eng.inputs:
        eng.host_array(nm)[...] = rng.random(eng.shapes[nm], dtype=np.float32)
    eng.upload_inputs()
    eng.forward_resident(2, use_graph=False)
    rows = eng.time_ops(reps=10)
    tot = sum(r[2] for r in rows)
    by_kind = {}
    for kind, name, ms, fl, by in rows:
        print("%-10s %-64s %8.1f us %7.1f TF/s %7.1f GB/s" % (kind, name[:64], ms * 1e3, fl / ms / 1e9 if ms else 0, by / ms / 1e6 if ms else 0))
        by_kind[kind] = by_kind.get(kind, 0.0) + ms
    print("total %.3f ms  " % tot + "  ".join("%s %.3f" % kv for kv in sorted(by_kind.items(), key=lambda kv: -kv[1])))
    if "inner_product" in by_kind:
        print("inner_product share of the forward: %.1f %%" % (100.0 * by_kind["inner_product"] / tot))
    eng.close()


if __name__ == "__main__":
    main()
