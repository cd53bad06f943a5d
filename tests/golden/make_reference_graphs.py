#!/usr/bin/env python3
"""Write tests/golden/reference_graphs.json: per-layer digests of the graphs the reference's net definitions parse to.

Needs a checkout of the reference (iKrishneel/fcn_object_detector), which the tests do not have: every prototxt is read
with this project's parser, reduced to tests/graph_signature.signature() and stored as one digest per layer plus the
input shapes.  Nothing of the files' text is stored.  The checks that need the files themselves are made here, when the
fixture is written: every net and solver definition of the reference parses, and the solver fields come out typed.

Usage:   python3 tests/golden/make_reference_graphs.py <reference checkout>
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

from fcn_object_detector_amd import proto  # noqa: E402
from graph_signature import layer_digests, signature  # noqa: E402

NETS = [("models/deploy.prototxt", "TEST"), ("models/train_val.prototxt", "TRAIN"), ("models/train_val2.prototxt", "TRAIN"),
        ("train/fcn_bbox/train_val.prototxt", "TRAIN"), ("train/bounding_box/train_val.prototxt", "TRAIN"),
        ("train/bounding_box/deploy.prototxt", "TEST")]
PARSE_ONLY = ["train/semantic_segmentation/train_val.prototxt", "train/fcn_bbox/solver.prototxt", "train/bounding_box/solver.prototxt"]


def main(ref: str) -> None:
    out = {}
    for rel, phase in NETS:
        inputs, layers = signature(proto.parse_file(os.path.join(ref, rel)), phase)
        out[rel] = {"phase": phase, "inputs": {k: list(v) for k, v in inputs.items()}, "layers": layer_digests(layers)}
    for rel in PARSE_ONLY:
        assert proto.parse_file(os.path.join(ref, rel)).fields, rel
    s = proto.parse_file(os.path.join(ref, "train/bounding_box/solver.prototxt"))
    assert s.get("solver_type") == "ADAM" and s.get("base_lr") == 1e-4 and s.get("stepsize") == 10000
    with open(os.path.join(HERE, "reference_graphs.json"), "w") as f:
        f.write("{\n" + ",\n".join("%s: %s" % (json.dumps(k), json.dumps(out[k], sort_keys=True)) for k in sorted(out)) + "\n}\n")      # a line per file
    print({k: len(v["layers"]) for k, v in out.items()})


if __name__ == "__main__":
    main(sys.argv[1])
