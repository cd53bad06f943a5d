"""`bench.py` without `--full` measures the headline and nothing else; `--full` adds every other measurement to the same line."""
import json
import os
import subprocess
import sys
import time

import pytest

from conftest import ROOT

BENCH = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1"]
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup", "n_gpus", "config", "repeats")
# what only a --full run measures: the forward's other figures ...
FORWARD_DETAILS = ("value_kernels_only", "kernels_only", "config2_frames_per_s", "config2_frames_per_s_in_flight", "config2_timed_region", "single_stream",
                   "pcie_inclusive_fps", "roofline", "roofline_in_flight")
# ... and the measurements of their own, which --no-cpu-baseline / --no-secondary / --no-train take out of a --full run again
OWN_RUNS = {"--no-cpu-baseline": ("cpu_baseline", "parity_rel_err", "speedup_vs_cpu", "speedup_vs_cpu_kernels_only"),
            "--no-secondary": ("detector_batch1", "forward_batch8", "inference_batch32", "secondary"),
            "--no-train": ("train",)}
OUTSIDE_STEPS_S = 30.0      # what a plain run may spend outside its warm-up and timed steps, start to exit


def run_bench(extra, timeout):
    t0 = time.perf_counter()
    r = subprocess.run(BENCH + extra, capture_output=True, text=True, timeout=timeout)
    wall = time.perf_counter() - t0
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 1      # ONE JSON line
    return json.loads(lines[0]), wall


def check_headline(line, steps, warmup):
    for k in HEADLINE:
        assert k in line, k
    assert line["metric"] == "frames/sec forward 448x448 @1 GPU; train imgs/sec @1/2/4/8 GPUs"
    assert line["unit"] == "frames/s" and line["higher_is_better"] is True and line["dtype"] == "f32"
    assert (line["steps"], line["warmup"], line["n_gpus"]) == (steps, warmup, 1)
    assert line["value"] > 0 and line["ms_per_step"] > 0
    assert abs(line["value"] * line["ms_per_step"] / 1e3 - 1.0) < 1e-3      # batch 1: frames/s and ms per step are the same measurement
    assert line["repeats"]["R"] == 5 and len(line["repeats"]["frames_per_s"]) == 5      # `value` is the median of --repeats windows of K steps


def test_per_launch_table_is_refused_without_full():
    """--per-op prints timings that only a --full run takes: asking for it alone is an error, before anything touches the GPU."""
    r = subprocess.run(BENCH + ["--steps", "1", "--per-op"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "--full" in r.stderr and r.stdout == ""


def test_full_is_documented_where_the_options_are():
    r = subprocess.run(BENCH + ["--help"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "--full" in r.stdout


@pytest.mark.gpu
def test_plain_run_measures_the_headline_only(gpu):
    line, wall = run_bench(["--steps", "40", "--warmup", "5"], timeout=300)
    check_headline(line, 40, 5)
    assert line["full"] is False
    for k in FORWARD_DETAILS + sum(OWN_RUNS.values(), ()):
        assert k not in line, k
    assert wall - (40 + 5) * line["ms_per_step"] / 1e3 < OUTSIDE_STEPS_S


@pytest.mark.gpu
def test_parts_of_a_full_run_can_be_left_out(gpu):
    """--full with its three measurements of their own switched off: the forward's other figures, timed around the headline's steps."""
    line, _ = run_bench(["--steps", "40", "--warmup", "5", "--full"] + sorted(OWN_RUNS), timeout=300)
    check_headline(line, 40, 5)
    assert line["full"] is True
    for k in FORWARD_DETAILS:
        assert k in line, k
    for k in sum(OWN_RUNS.values(), ()):
        assert k not in line, k
    assert line["kernels_only"]["frames_per_s"] == line["value_kernels_only"] > 0 and len(line["kernels_only"]["repeats"]) == 5
    assert line["config2_frames_per_s_in_flight"] == line["value"] and line["config2_frames_per_s"] > 0
    assert line["single_stream"]["frames_per_s"] > 0 and line["single_stream"]["device_ms_per_step"] > 0
    assert line["roofline"]["bound"] == "mfma" and 0 < line["roofline"]["frac"] < 1 and line["roofline"]["live_back_to_back"]["achieved"] > 0


@pytest.mark.gpu
def test_full_run_measures_everything(gpu):
    """The whole --full line: CPU baseline with its parity check, detector per camera frame, training step, batch-8 / batch-32 / half-float
    forwards and the VGG16-FCN net behind the same headline."""
    line, wall = run_bench(["--steps", "40", "--warmup", "5", "--full", "--train-steps", "3"], timeout=600)
    check_headline(line, 40, 5)
    assert line["full"] is True and wall < 600
    for k in FORWARD_DETAILS + sum(OWN_RUNS.values(), ()):
        assert k in line, k
    assert line["cpu_baseline"]["value"] > 0 and max(line["parity_rel_err"].values()) < 1e-3
    assert "error" not in line["train"] and line["train"]["imgs_per_s"] > 0 and "error" not in line["train"]["with_data_layer"]
    assert line["detector_batch1"]["frames_per_s_4_in_flight"] > 0 and line["forward_batch8"]["frames_per_s"] > 0
    assert line["inference_batch32"]["f16"]["frames_per_s"] > 0 and line["inference_batch32"]["f32"]["frames_per_s"] > 0
    assert max(line["inference_batch32"]["f16"]["rel_err_vs_f32"].values()) < 5e-2
    assert line["secondary"]["forward_448_b1"]["frames_per_s"] > 0 and line["secondary"]["train_288_b24"]["imgs_per_s"] > 0
