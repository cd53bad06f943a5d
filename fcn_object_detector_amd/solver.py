"""Solver front end: what ``caffe train --solver=... [--weights=...|--snapshot=...] --gpu=...`` does
(reference: train/train.sh:25-28, with the solver.prototxt files under models/), on top of TrainEngine.

Mirrors Caffe's Solver: Step() = forward/backward + update, ``display`` lines with the smoothed loss and the
net outputs, test nets every ``test_interval`` iterations (Solver::Test: ``test_iter`` forwards of a TEST-phase net that reads
the training net's weights in place, scores summed on the device), ``snapshot`` every N iterations as ``<prefix>_iter_<N>.caffemodel`` + ``.solverstate``, resume from a
``.solverstate``.  Multi-GPU (new: the reference is single-GPU) is data parallel, one process per GPU, gradients
summed with RCCL by TrainEngine.
"""
from __future__ import annotations

import ctypes as C
import os
import sys
import time
from collections import OrderedDict, deque
from typing import Callable, Dict, List, Optional

import numpy as np

from . import lib as L
from . import proto
from . import pylayer
from .engine import Engine
from .netspec import NetSpec, fill_params
from .train import SolverParams, TrainEngine


def _resolve(path: str, anchor: str) -> str:
    """Caffe resolves paths against the working directory; fall back to the directory of the file that names them."""
    if os.path.isabs(path) or os.path.isfile(path):
        return path
    alt = os.path.join(os.path.dirname(os.path.abspath(anchor)), path)
    return alt if os.path.isfile(alt) else path


def _log(msg: str) -> None:
    sys.stderr.write(time.strftime("I%m%d %H:%M:%S ") + msg + "\n")
    sys.stderr.flush()


class _BlobView(object):
    def __init__(self, eng: TrainEngine, name: str):
        self._eng, self._name = eng, name

    @property
    def data(self) -> np.ndarray:
        return self._eng.read_blob(self._name)

    @property
    def diff(self) -> np.ndarray:
        return self._eng.read_grad(self._name)

    @property
    def shape(self):
        return tuple(self._eng.shapes[self._name])


class _ParamView(object):
    def __init__(self, solver: "Solver", layer: str, index: int):
        self._s, self._layer, self._index = solver, layer, index

    @property
    def data(self) -> np.ndarray:
        return self._s.engine.download_params()[self._layer][self._index]

    @property
    def diff(self) -> np.ndarray:
        return self._s.engine.download_grads()[self._layer][self._index]


class TrainNet(object):
    """``solver.net``: read access to blobs / params of the training net, ``copy_from`` and ``save``."""

    def __init__(self, solver: "Solver"):
        self._s = solver
        eng = solver.engine
        self.blobs = OrderedDict((n, _BlobView(eng, n)) for n in eng.shapes)
        self.params = OrderedDict((l.name, [_ParamView(solver, l.name, i) for i in range(len(eng.params_host[l.name]))])
                                  for l in eng.spec.param_layers())

    def copy_from(self, weights_path: str) -> None:
        """Net::CopyTrainedLayersFrom: by layer name; layers absent from the file keep their filler values."""
        if not os.path.isfile(weights_path):
            raise IOError("weights file not found: %s" % weights_path)
        eng = self._s.engine
        proto.copy_trained_layers(weights_path, eng.params_host, eng.set_params, log=self._s.log)

    def save(self, path: str) -> None:
        self._s.engine.save(path)


class _TestParamView(object):
    def __init__(self, eng: Engine, layer: str, index: int):
        self._eng, self._layer, self._index = eng, layer, index

    @property
    def data(self) -> np.ndarray:
        return self._eng.read_param(self._layer, self._index)


class TestNet(object):
    """One scoring net (an entry of ``solver.test_nets``; `caffe test` builds one on its own): a TEST-phase engine with the
    accumulation launches behind its last layer, its own Python-layer instances feeding THAT engine, and - inside a solver -
    the training engine's parameters read in place.  ``.blobs[name].data``, ``.params[layer][i].data``, ``.forward()``."""

    __test__ = False      # (not a pytest class, whatever the name says)

    def __init__(self, net_file: str, device: int = 0, autotune: bool = True, share_params: Optional[Engine] = None, params=None):
        self.net_file = net_file
        msg = proto.parse_file(net_file)
        spec = NetSpec.public(msg, "TEST")
        self.py_layers, data_shapes = pylayer.setup_python_layers(spec, pylayer.TEST)
        spec = NetSpec.public(msg, "TEST")
        spec.infer({**spec.input_shapes, **data_shapes})
        self.engine = eng = Engine(spec, data_shapes, params, device=device, autotune=autotune, share_params=share_params,
                                   score_outputs=True)
        self._device_label_tops = {}
        for l, inst, bottoms, tops in self.py_layers:      # as the training net's layers are bound to the training engine
            if getattr(inst, "supports_device_scenes", False):
                inst.bind_device(eng, [t.name for t in tops])
                eng.device_fed |= set(inst.device_tops)
            if getattr(inst, "supports_device_targets", False) and getattr(inst, "mode", None) == "detectnet" and len(tops) >= 6:
                inst.device_targets = True
                self._device_label_tops[id(inst)] = tuple(t.name for t in tops[1:6])
                eng.device_fed |= set(self._device_label_tops[id(inst)])      # generated in HBM by set_targets(): never uploaded
        self.host_fed = any(nm not in eng.device_fed for nm in eng.inputs)
        self._uploaded = C.c_void_p()
        L.call("fcn_event_create", C.byref(self._uploaded))
        self.blobs = OrderedDict((n, _BlobView(eng, n)) for n in eng.shapes)
        self.params = OrderedDict((l.name, [_TestParamView(eng, l.name, i) for i in range(len(eng.params_host[l.name]))])
                                  for l in eng.spec.param_layers())
        self.outputs = list(eng.outputs)

    def feed(self) -> None:
        """The next batch of every Python layer into this net's engine (host arrays, or rendered / generated in HBM)."""
        eng = self.engine
        for l, inst, bottoms, tops in self.py_layers:
            inst.reshape(bottoms, tops)
            inst.forward(bottoms, tops)
            label_tops = self._device_label_tops.get(id(inst), ())
            for t in tops:
                if tuple(t.shape_) != tuple(eng.shapes[t.name]):
                    raise NotImplementedError("Python layer %s changed the shape of %s" % (l.name, t.name))
                if t.name not in eng.device_fed:
                    eng.host_array(t.name)[...] = t.data
            if label_tops:
                eng.set_targets(inst.last_rects, inst.last_labels, inst.stride, tops=label_tops)

    def forward(self) -> Dict[str, np.ndarray]:
        """One batch, outputs downloaded (pycaffe's ``net.forward()``)."""
        self.feed()
        return {k: v.copy() for k, v in self.engine.forward().items()}

    def copy_from(self, weights_path: str, log=None) -> None:
        eng = self.engine
        proto.copy_trained_layers(weights_path, eng.params_host, eng.set_params, log=log)

    def run_pass(self, iters: int, per_batch: Optional[Callable[[int, Dict[str, np.ndarray]], None]] = None) -> Dict[str, np.ndarray]:
        """`iters` forwards whose output blobs are summed on the device; returns {blob: float32 sums, blob shape}.  Without
        per_batch nothing is read back before the end and the host waits for the device only where a host-fed input array is about
        to be refilled; with it (`caffe test` prints every batch) each forward downloads its outputs."""
        eng = self.engine
        eng.score_begin(io=per_batch is not None)
        for k in range(int(iters)):
            if per_batch is not None:
                self.feed()
                per_batch(k, eng.forward())
                continue
            if self.host_fed and k:
                L.call("fcn_event_sync", self._uploaded)      # the copy out of the pinned input arrays has been taken
            self.feed()
            eng.forward_score(self._uploaded if self.host_fed else None)
        return eng.score_read()

    def lines(self, sums: Dict[str, np.ndarray], iters: int, fmt: str) -> List[str]:
        """Caffe's result lines: one per element of every output blob (net order, NCHW order), `fmt` % (index, blob, mean), with
        ` (* w = w*mean loss)` on blobs that carry a loss weight."""
        out, j = [], 0
        for nm in self.outputs:
            w = self.engine.loss_blobs.get(nm, 0.0)
            for v in (sums[nm] / np.float32(iters)).reshape(-1):
                out.append(fmt % (j, nm, v) + (" (* %g = %g loss)" % (w, w * v) if w else ""))
                j += 1
        return out

    def close(self) -> None:
        self.engine.close()


class Solver(object):
    TYPE_NAMES = {"SGD": "SGD", "NESTEROV": "Nesterov", "ADAGRAD": "AdaGrad", "RMSPROP": "RMSProp", "ADADELTA": "AdaDelta", "ADAM": "Adam"}

    def __init__(self, solver_file: str, device: int = 0, comm=None, rank: int = 0, log: Optional[Callable[[str], None]] = _log,
                 autotune: bool = True):
        if not os.path.isfile(str(solver_file)):
            raise IOError("solver file not found: %s" % solver_file)
        self.solver_file = str(solver_file)
        self.param = SolverParams(proto.parse_file(self.solver_file))
        if not self.param.net:
            raise ValueError("%s: solver needs a `net:` (or `train_net:`) entry" % solver_file)
        self.net_file = _resolve(str(self.param.net), self.solver_file)
        if not os.path.isfile(self.net_file):
            raise IOError("net file not found: %s" % self.param.net)
        self.rank, self.comm, self.device = int(rank), comm, int(device)
        self.log = log if (log is not None and self.rank == 0) else (lambda m: None)
        L.call("fcn_init", self.device)
        msg = proto.parse_file(self.net_file)
        spec = NetSpec.public(msg, "TRAIN")
        self.py_layers, data_shapes = pylayer.setup_python_layers(spec, pylayer.TRAIN)
        spec = NetSpec.public(msg, "TRAIN")
        spec.infer({**spec.input_shapes, **data_shapes})
        self.engine = TrainEngine(spec, data_shapes, fill_params(spec, seed=0), device=self.device, solver=self.param, comm=comm,
                                  autotune=autotune)
        self.net = TrainNet(self)
        self._losses: deque = deque(maxlen=max(self.param.average_loss, 1))
        self._fed = False
        self._device_label_tops = {}
        for l, inst, bottoms, tops in self.py_layers:
            # a data layer that can render its scenes on the device writes `data` (and HEAD's class mask) straight into HBM
            if getattr(inst, "supports_device_scenes", False):
                inst.bind_device(self.engine, [t.name for t in tops])
                self.engine.device_fed |= set(inst.device_tops)
            # a data layer that can hand over ground-truth boxes gets its label grids generated in HBM (fcn_gen_targets_nhwc)
            if getattr(inst, "supports_device_targets", False) and getattr(inst, "mode", None) == "detectnet" and len(tops) >= 6:
                inst.device_targets = True
                self._device_label_tops[id(inst)] = tuple(t.name for t in tops[1:6])
        # Solver::InitTestNets: one scoring net per instance, on rank 0 only (Caffe's root solver tests); each reads this engine's
        # flat parameter buffer in place
        self.test_nets: List[TestNet] = []
        self.test_results: List[Optional[Dict[str, np.ndarray]]] = []
        if self.rank == 0:
            for path, _iters in self.param.test_instances:
                path = _resolve(path, self.solver_file)
                if not os.path.isfile(path):
                    raise IOError("test net file not found: %s" % path)
                self.test_nets.append(TestNet(path, device=self.device, autotune=autotune, share_params=self.engine))
                self.test_results.append(None)
        self._ev_trained, self._ev_tested = C.c_void_p(), C.c_void_p()
        if self.test_nets:
            L.call("fcn_event_create", C.byref(self._ev_trained))
            L.call("fcn_event_create", C.byref(self._ev_tested))
        self.log("Solver: %s, net %s, %d learnable floats, world %d" % (
            self.param.kind, self.net_file, self.engine.param_count, comm.world if comm is not None else 1))
        p = self.param
        self.log('Initializing solver from parameters: type: "%s" lr_policy: "%s" base_lr: %g regularization_type: "%s" iter_size: %d '
                 'clip_gradients: %g' % (self.TYPE_NAMES[p.kind], p.lr_policy, p.base_lr, p.regularization_type, p.iter_size, p.clip_gradients))

    @property
    def iter(self) -> int:
        return self.engine.iter

    # ------------------------------------------------------------------ Solver::Step
    def _feed(self) -> None:
        eng = self.engine
        for l, inst, bottoms, tops in self.py_layers:
            inst.reshape(bottoms, tops)
            inst.forward(bottoms, tops)
            label_tops = self._device_label_tops.get(id(inst), ()) if getattr(inst, "device_targets", False) else ()
            for t in tops:
                if tuple(t.shape_) != tuple(eng.shapes[t.name]):
                    raise NotImplementedError("Python layer %s changed the shape of %s" % (l.name, t.name))
                if t.name not in label_tops and t.name not in getattr(inst, "device_tops", ()):
                    eng.host_array(t.name)[...] = t.data
            if label_tops:
                eng.set_targets(inst.last_rects, inst.last_labels, inst.stride, tops=label_tops)

    def _all_device_fed(self) -> bool:
        """True when no top of any Python layer travels through a host array (scenes composed and labels generated in HBM):
        the next batch can then be planned and enqueued while the device is still busy with the current iteration."""
        for l, inst, bottoms, tops in self.py_layers:
            label_tops = self._device_label_tops.get(id(inst), ()) if getattr(inst, "device_targets", False) else ()
            if any(t.name not in label_tops and t.name not in getattr(inst, "device_tops", ()) for t in tops):
                return False
        return bool(self.py_layers)

    # ------------------------------------------------------------------ Solver::Test
    def test(self, i: int = 0) -> Dict[str, np.ndarray]:
        """Solver::Test(i): test_iter[i] forwards of test net i on the current weights; returns {output blob: float32 mean over the
        forwards} (also kept in ``test_results[i]``).  The pass is ordered against training with events only: it starts behind
        everything queued on the training stream (the previous update) and the training stream waits for its last launch."""
        net, iters = self.test_nets[i], self.param.test_instances[i][1]
        self.log("Iteration %d, Testing net (#%d)" % (self.iter, i))
        L.call("fcn_init", self.device)
        L.call("fcn_event_record", self._ev_trained, self.engine.stream)
        L.call("fcn_stream_wait_event", net.engine.stream, self._ev_trained)
        sums = net.run_pass(iters)
        L.call("fcn_event_record", self._ev_tested, net.engine.stream)
        L.call("fcn_stream_wait_event", self.engine.stream, self._ev_tested)
        means = {nm: (sums[nm] / np.float32(iters)).astype(np.float32) for nm in net.outputs}
        if self.param.test_compute_loss:
            self.log("Test loss: %g" % sum(w * float(means[nm].sum()) for nm, w in net.engine.loss_blobs.items() if nm in means))
        for line in net.lines(sums, iters, "    Test net output #%d: %s = %g"):
            self.log(line)
        self.test_results[i] = means
        return means

    def test_all(self) -> List[Dict[str, np.ndarray]]:
        return [self.test(i) for i in range(len(self.test_nets))]

    def step(self, iters: int = 1, pipeline: bool = False) -> Dict[str, float]:
        """Solver::Step.  pipeline=True (what solve() / `caffe train` use) plans and enqueues the next batch while the device
        runs the current iteration; it is off by default because the input blobs then already hold the NEXT batch when
        step() returns, which a pycaffe caller inspecting net.blobs would not expect."""
        p, out = self.param, {}
        stop = self.iter + int(iters)
        pipelined = pipeline and self._all_device_fed()
        while self.iter < stop:
            it = self.iter
            if self.test_nets and p.test_due(it):
                self.test_all()
            for j in range(p.iter_size):      # iter_size passes, each on a fresh batch; the engine updates after the last one
                if not self._fed:
                    self._feed()
                self._fed = False
                self.engine.step_begin()
                if pipelined and (j + 1 < p.iter_size or it + 1 < p.max_iter):
                    # the renders of the next batch queue up behind this iteration on the stream; its planning (host RNG and
                    # box bookkeeping) overlaps the device work
                    self._feed()
                    self._fed = True
                out = self.engine.step_end()
            self._losses.append(out["total_loss"])
            if p.display and it % p.display == 0:
                self.log("Iteration %d, loss = %g" % (it, sum(self._losses) / len(self._losses)))
                for j, (name, w) in enumerate(self.engine.loss_blobs.items()):
                    self.log("    Train net output #%d: %s = %g (* %g = %g loss)" % (j, name, out[name], w, w * out[name]))
                self.log("Iteration %d, lr = %g" % (it, p.rate(it)))
            if not np.isfinite(out["total_loss"]):
                raise FloatingPointError("loss is %r at iteration %d" % (out["total_loss"], it))
            if p.snapshot and self.iter % p.snapshot == 0:
                self.snapshot()
        return out

    def solve(self, resume_file: Optional[str] = None) -> None:
        if resume_file:
            self.restore(resume_file)
        self.log("Solving %s" % (self.engine.spec.name or os.path.basename(self.net_file)))
        self.step(max(self.param.max_iter - self.iter, 0), pipeline=True)
        if not (self.param.snapshot and self.iter % self.param.snapshot == 0):
            self.snapshot()
        if self.test_nets and self.param.test_interval and self.iter % self.param.test_interval == 0:
            self.test_all()
        self.log("Optimization Done.")

    # ------------------------------------------------------------------ snapshots
    def snapshot_filename(self, ext: str) -> str:
        return "%s_iter_%d%s" % (self.param.snapshot_prefix, self.iter, ext)

    def snapshot(self) -> Optional[str]:
        if self.rank != 0:
            return None
        model, state = self.snapshot_filename(".caffemodel"), self.snapshot_filename(".solverstate")
        d = os.path.dirname(model)
        if d:
            os.makedirs(d, exist_ok=True)
        self.log("Snapshotting to binary proto file %s" % model)
        self.engine.save(model)
        self.log("Snapshotting solver state to binary proto file %s" % state)
        with open(state, "wb") as f:
            f.write(proto.pack_solverstate(self.iter, self.engine.download_history(), learned_net=model))
        return model

    def restore(self, state_file: str) -> None:
        if not os.path.isfile(state_file):
            raise IOError("solver state not found: %s" % state_file)
        with open(state_file, "rb") as f:
            it, history, learned = proto.unpack_solverstate(f.read(), with_learned_net=True)
        self.engine.upload_history(history)      # (first: a state written by another solver type is refused before anything is loaded)
        if learned:
            self.net.copy_from(_resolve(learned, state_file))
        self.engine.iter = int(it)
        self.log("Restoring previous solver status from %s (iteration %d)" % (state_file, it))

    def close(self) -> None:
        for net in self.test_nets:
            net.close()
        self.engine.close()


SGDSolver = Solver
AdamSolver = Solver
NesterovSolver = AdaGradSolver = RMSPropSolver = AdaDeltaSolver = Solver


def get_solver(solver_file: str, **kw) -> Solver:
    return Solver(solver_file, **kw)
