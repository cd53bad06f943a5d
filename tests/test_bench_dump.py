"""`bench.py --dump-outputs DIR`: the arrays the last timed step returned, as DIR/<blob>.npy."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, rel_err

BENCH = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--no-cpu-baseline", "--no-train", "--no-secondary", "--repeats", "1"]


def test_dump_larger_than_the_limit_is_refused_before_anything_runs(tmp_path):
    r = subprocess.run(BENCH + ["--steps", "1", "--batch", "1100", "--dump-outputs", str(tmp_path / "dump")], capture_output=True, text=True)
    assert r.returncode != 0 and "at most 64 MB" in r.stderr
    assert not (tmp_path / "dump").exists()


@pytest.mark.gpu
def test_dump_holds_the_outputs_of_the_last_timed_step(gpu, tmp_path):
    """Config 2's region (outputs read back into host arrays) and the kernels-only region (outputs left in HBM) run the same
    forward on the same seeded frame and weights: both dumps hold the two head blobs as float32, and they agree (each
    process tunes its own tile plan, so the sums may differ in their order: last bits, not more)."""
    dumps = []
    for name, extra in (("io", []), ("resident", ["--no-io-region"])):
        d = tmp_path / name
        r = subprocess.run(BENCH + ["--steps", "7", "--warmup", "2", "--dump-outputs", str(d)] + extra, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        line = json.loads(r.stdout.strip().splitlines()[-1])
        assert line["steps"] == 7 and line["dumped_outputs"]["arrays"] == {"coverage": [1, 4, 28, 28], "bboxes": [1, 16, 28, 28]}
        assert sorted(os.listdir(d)) == ["bboxes.npy", "coverage.npy"]
        dumps.append({k: np.load(d / (k + ".npy")) for k in ("coverage", "bboxes")})
        for k, shape in (("coverage", (1, 4, 28, 28)), ("bboxes", (1, 16, 28, 28))):
            a = dumps[-1][k]
            assert a.dtype == np.float32 and a.shape == shape and np.isfinite(a).all() and np.abs(a).max() > 0
    for k in ("coverage", "bboxes"):
        assert rel_err(dumps[0][k], dumps[1][k]) < 1e-4
