#!/usr/bin/python3
"""`caffe` command-line tool over the MI355X engine — the binary the reference's training script runs
(reference: train/train.sh:25-28, `$CAFFE_ROOT/build/tools/caffe train --solver=... --gpu=0 --weights=...`).
The build installs this file as <repo>/fcn_object_detector_amd/build/tools/caffe (csrc/Makefile, beside libfcnhip.so, which the
tool cannot run without): point CAFFE_ROOT at <repo>/fcn_object_detector_amd and that script works unchanged.

    caffe train --solver=solver.prototxt [--weights=a.caffemodel[,b.caffemodel]] [--snapshot=x.solverstate] [--gpu=0|0,1,..|all]
    caffe test --model=train_val.prototxt --weights=a.caffemodel [--iterations=50] [--gpu=0]
    caffe time --model=deploy.prototxt [--iterations=50] [--gpu=0]      (FCN_DTYPE=f16: the half-float engine)
    caffe device_query [--gpu=0]

With more than one GPU the tool starts one process per GPU (data parallel, gradients summed over RCCL); it can
also be launched as the ranks of `python -m torch.distributed.run` (RANK / LOCAL_RANK / WORLD_SIZE in the environment).
"""
import os
import subprocess
import sys

_REPO = os.path.dirname(os.path.abspath(__file__))      # (the installed copy lies three levels below the repository, this file one)
while not os.path.isdir(os.path.join(_REPO, "fcn_object_detector_amd", "python")) and os.path.dirname(_REPO) != _REPO:
    _REPO = os.path.dirname(_REPO)
for p in (_REPO, os.path.join(_REPO, "fcn_object_detector_amd", "python")):
    if p not in sys.path:
        sys.path.insert(0, p)

USAGE = __doc__.split("\n\n")[1]


def parse_flags(argv):
    """gflags style: --name=value, -name=value, --name value; returns (positional, flags)."""
    pos, flags, i = [], {}, 0
    while i < len(argv):
        a = argv[i]
        if a.startswith("-"):
            name = a.lstrip("-")
            if "=" in name:
                name, val = name.split("=", 1)
            elif i + 1 < len(argv) and not argv[i + 1].startswith("-"):
                val = argv[i + 1]
                i += 1
            else:
                val = "true"
            flags[name.replace("-", "_")] = val
        else:
            pos.append(a)
        i += 1
    return pos, flags


def device_count():
    """Counted in a helper process so that this launcher never initialises the GPU itself."""
    code = ("import sys; sys.path.insert(0, %r); import ctypes; from fcn_object_detector_amd import lib as L; "
            "n = ctypes.c_int(0); L.call('fcn_device_count', ctypes.byref(n)); print(n.value)" % _REPO)
    return int(subprocess.check_output([sys.executable, "-c", code]).decode().strip().splitlines()[-1])


def gpu_list(flag):
    if flag is None or flag == "":
        return [0]
    if flag == "all":
        return list(range(device_count()))
    return [int(g) for g in flag.split(",") if g != ""]


def cmd_train(flags):
    if "solver" not in flags:
        sys.stderr.write("Need a solver definition to train.\n")
        return 1
    if "snapshot" in flags and "weights" in flags:
        sys.stderr.write("Give a snapshot to resume training or weights to finetune but not both.\n")
        return 1
    ranked = "RANK" in os.environ and int(os.environ.get("WORLD_SIZE", "1")) > 1
    gpus = gpu_list(flags.get("gpu"))
    if not ranked and len(gpus) > 1:
        return spawn_ranks(gpus)

    from fcn_object_detector_amd import dp
    from fcn_object_detector_amd.solver import Solver
    rank, world = (dp.env_rank(), dp.env_world_size()) if ranked else (0, 1)
    device = dp.env_device() if ranked else gpus[0]
    cp = comm = None
    if world > 1:
        cp = dp.ControlPlane()
        comm = dp.RcclComm(cp, device)
    os.environ.setdefault("FCN_DATA_SEED", str(1 + rank))
    solver = Solver(flags["solver"], device=device, comm=comm, rank=rank)
    if "weights" in flags:
        for w in flags["weights"].split(","):
            solver.log("Finetuning from %s" % w)
            solver.net.copy_from(w)
    solver.solve(resume_file=flags.get("snapshot"))
    if cp is not None:
        cp.barrier()
        comm.close()
        cp.close()
    solver.close()
    return 0


def spawn_ranks(gpus):
    from fcn_object_detector_amd import dp      # (imports nothing that touches the GPU)
    return dp.spawn_ranks(__file__, sys.argv[1:], gpus, {})


def cmd_test(flags):
    """Score a snapshot: `iterations` batches of the model's TEST phase, every output blob summed on the device (the solver's test
    pass), Caffe's lines per batch and for the means.  $FCN_AUTOTUNE=0 keeps the default launch plan (repeatable bits)."""
    if "model" not in flags:
        sys.stderr.write("Need a model definition to score.\n")
        return 1
    if "weights" not in flags:
        sys.stderr.write("Need model weights to score.\n")
        return 1
    for f in (flags["model"], flags["weights"]):
        if not os.path.isfile(f):
            sys.stderr.write("file not found: %s\n" % f)
            return 1
    from fcn_object_detector_amd import lib as L
    from fcn_object_detector_amd.solver import TestNet, _log
    iters = int(flags.get("iterations", 50))
    device = gpu_list(flags.get("gpu"))[0]
    L.call("fcn_init", device)
    net = TestNet(flags["model"], device=device, autotune=os.environ.get("FCN_AUTOTUNE", "1") != "0")
    net.copy_from(flags["weights"], log=_log)
    _log("Running for %d iterations." % iters)
    weights = net.engine.loss_blobs
    loss = [0.0]

    def per_batch(k, out):
        for nm in net.outputs:
            for v in out[nm].reshape(-1):
                _log("Batch %d, %s = %g" % (k, nm, v))
            if nm in weights:
                loss[0] += weights[nm] * float(out[nm].sum())

    sums = net.run_pass(iters, per_batch)
    _log("Loss: %g" % (loss[0] / iters))
    for line in net.lines(sums, iters, "%.0s%s = %g"):
        _log(line)
    net.close()
    return 0


def cmd_time(flags):
    import numpy as np
    from fcn_object_detector_amd import lib as L, proto
    from fcn_object_detector_amd.engine import Engine
    from fcn_object_detector_amd.netspec import NetSpec
    if "model" not in flags:
        sys.stderr.write("Need a model definition to time.\n")
        return 1
    iters = int(flags.get("iterations", 50))
    device = gpu_list(flags.get("gpu"))[0]
    L.call("fcn_init", device)
    spec = NetSpec.public(proto.parse_file(flags["model"]), "TEST")
    eng = Engine(spec, data_shapes={}, params=None, device=device, dtype=os.environ.get("FCN_DTYPE", "f32"))      # (as caffe.Net reads it)
    rng = np.random.default_rng(0)
    for nm in eng.inputs:
        eng.host_array(nm)[...] = rng.random(eng.shapes[nm], dtype=np.float32) * 255
    eng.forward()
    ms = eng.forward_resident(iters) / iters
    for kind, name, t, _flops, _bytes in eng.time_ops(max(iters // 5, 3)):
        sys.stderr.write("%28s\tforward: %g ms.\n" % (name, t))
    sys.stderr.write("Average Forward pass: %g ms.\n" % ms)
    eng.close()
    return 0


def cmd_device_query(flags):
    import ctypes
    from fcn_object_detector_amd import lib as L
    for g in gpu_list(flags.get("gpu")):
        L.call("fcn_init", g)
        buf = ctypes.create_string_buffer(256)
        L.call("fcn_device_name", buf, 256)
        sys.stderr.write("Device id: %d\nName: %s\n" % (g, buf.value.decode()))
    return 0


def main(argv):
    pos, flags = parse_flags(argv)
    if not pos or pos[0] not in ("train", "test", "time", "device_query"):
        sys.stderr.write("usage:\n" + USAGE + "\n")
        return 1
    return {"train": cmd_train, "test": cmd_test, "time": cmd_time, "device_query": cmd_device_query}[pos[0]](flags)


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
