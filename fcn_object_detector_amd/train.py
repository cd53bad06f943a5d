"""Training step on the device: Net::ForwardBackward + solver update, optionally data-parallel.

Stands in for `caffe train` (reference: train/train.sh:25-28) over the DetectNet training net
(reference: models/train_val.prototxt with the Python data layer's tops, README.md:57-76) and the
settings a solver.prototxt may carry: every solver type and learning-rate policy of Caffe's
SolverParameter, L1 / L2 weight decay, clip_gradients, iter_size, per-blob lr_mult / decay_mult.

Data layout: every blob that receives a gradient has a gradient buffer with the SAME NHWC view
geometry as its activation (so Concat / Slice / Dropout views need no backward kernel); all
parameter gradients live in one flat buffer parallel to `Engine.param_flat`, which is what the
solver kernel updates and what the RCCL all-reduce sums across ranks in one call.
"""
from __future__ import annotations

import ctypes as C
import os
import math
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import lib as L
from . import proto
from . import storage as S
from .backward import BackwardPlanner
from .engine import Blob, DevView, DeviceBuffer, Engine, Op, PinnedArray, _r4, graphs_enabled
from .netspec import DATA_TYPES, Layer, NetSpec

F32 = np.float32


class SolverParams:
    """Caffe's SolverParameter as far as `caffe train` on one training net needs it: every solver type, every lr_policy, L1 / L2
    regularisation, clip_gradients and iter_size, and the test-net schedule (test_iter / test_interval / test_net,
    Solver::InitTestNets: `test_instances` lists what the solver scores, `test_due(it)` says when).

        type          histories  update (g' = normalised, clipped gradient + regularisation; lr = rate(iter) * lr_mult)
        SGD           1          h = momentum*h + lr*g' ; w -= h
        Nesterov      1          h_old = h ; h = momentum*h + lr*g' ; w -= (1+momentum)*h - momentum*h_old
        AdaGrad       1          h += g'^2 ; w -= lr*g' / (sqrt(h) + delta)                            (momentum must be 0)
        RMSProp       1          h = rms_decay*h + (1-rms_decay)*g'^2 ; w -= lr*g' / (sqrt(h) + delta)  (momentum must be 0)
        AdaDelta      2          h1 = momentum*h1 + (1-momentum)*g'^2 ; u = g'*sqrt((h2+delta)/(h1+delta)) ;
                                 h2 = momentum*h2 + (1-momentum)*u^2 ; w -= lr*u
        Adam          2          m, v moments ; w -= lr*sqrt(1-momentum2^t)/(1-momentum^t) * m / (sqrt(v) + delta)
    """

    KINDS = ("SGD", "NESTEROV", "ADAGRAD", "RMSPROP", "ADADELTA", "ADAM")
    POLICIES = ("fixed", "step", "exp", "inv", "multistep", "poly", "sigmoid")

    def __init__(self, msg: Optional[proto.Msg] = None, **kw):
        g = (lambda k, d=None: msg.get(k, d)) if msg is not None else (lambda k, d=None: d)
        self.net = g("net", g("train_net"))
        self.base_lr = float(kw.get("base_lr", g("base_lr", 0.01)))
        self.momentum = float(kw.get("momentum", g("momentum", 0.0)))
        self.momentum2 = float(kw.get("momentum2", g("momentum2", 0.999)))
        self.rms_decay = float(kw.get("rms_decay", g("rms_decay", 0.99)))
        self.delta = float(kw.get("delta", g("delta", 1e-8)))
        self.weight_decay = float(kw.get("weight_decay", g("weight_decay", 0.0)))
        self.regularization_type = str(kw.get("regularization_type", g("regularization_type", "L2")))
        self.clip_gradients = float(kw.get("clip_gradients", g("clip_gradients", -1.0)))
        self.lr_policy = str(kw.get("lr_policy", g("lr_policy", "fixed")))
        self.gamma = float(kw.get("gamma", g("gamma", 0.1)))
        self.power = float(kw.get("power", g("power", 0.0)))
        self.stepsize = int(kw.get("stepsize", g("stepsize", 1)))
        self.stepvalue = sorted(int(v) for v in kw.get("stepvalue", msg.getall("stepvalue") if msg is not None else ()))
        self.max_iter = int(kw.get("max_iter", g("max_iter", 1)))
        self.iter_size = int(kw.get("iter_size", g("iter_size", 1)))
        self.display = int(kw.get("display", g("display", 0)))
        self.average_loss = int(kw.get("average_loss", g("average_loss", 1)))
        self.snapshot = int(kw.get("snapshot", g("snapshot", 0)))
        self.snapshot_prefix = str(kw.get("snapshot_prefix", g("snapshot_prefix", "snapshot")))
        # `type: "Nesterov"` (a string, any case) or the older enum `solver_type: NESTEROV`
        kind = kw.get("solver_type", kw.get("type", g("solver_type", g("type", "SGD"))))
        self.kind = str(kind).upper()
        if self.kind not in self.KINDS:
            raise ValueError("type: unknown solver type %r (one of SGD, Nesterov, AdaGrad, RMSProp, AdaDelta, Adam)" % str(kind))
        if self.lr_policy not in self.POLICIES:
            raise ValueError("lr_policy: unknown policy %r (one of %s)" % (self.lr_policy, ", ".join(self.POLICIES)))
        if self.regularization_type not in ("L1", "L2"):
            raise ValueError("regularization_type: %r is neither \"L1\" nor \"L2\"" % self.regularization_type)
        if self.kind in ("ADAGRAD", "RMSPROP") and self.momentum != 0.0:
            raise ValueError("momentum: cannot be used with %s (it must be 0)" % {"ADAGRAD": "AdaGrad", "RMSPROP": "RMSProp"}[self.kind])
        if not 0.0 <= self.momentum < 1.0:
            raise ValueError("momentum: %g is outside [0, 1)" % self.momentum)
        if not 0.0 <= self.rms_decay < 1.0:
            raise ValueError("rms_decay: %g is outside [0, 1)" % self.rms_decay)
        if self.lr_policy == "multistep" and not self.stepvalue:
            raise ValueError("stepvalue: lr_policy \"multistep\" needs at least one")
        if self.lr_policy == "poly" and self.max_iter <= 0:
            raise ValueError("max_iter: lr_policy \"poly\" needs max_iter > 0")
        if self.lr_policy in ("step", "sigmoid") and self.stepsize <= 0:
            raise ValueError("stepsize: lr_policy \"%s\" needs stepsize > 0" % self.lr_policy)
        if self.iter_size < 1:
            raise ValueError("iter_size: %d is not positive" % self.iter_size)
        # ---- test nets (Solver::InitTestNets): the test_net files in order, then the `net:` file in TEST phase once for every
        # test_iter entry left over; one test_iter per instance; test_interval > 0 as soon as there is one
        rep = (lambda k: list(kw[k]) if k in kw else (list(msg.getall(k)) if msg is not None else []))
        for k in ("test_state", "net_param", "train_net_param", "test_net_param"):
            if k in kw or (msg is not None and msg.getall(k)):
                raise ValueError("%s: not supported (name the nets by file: net / train_net / test_net)" % k)
        self.train_net = kw.get("train_net", g("train_net"))
        self.test_iter = [int(v) for v in rep("test_iter")]
        self.test_net = [str(v) for v in rep("test_net")]
        self.test_interval = int(kw.get("test_interval", g("test_interval", 0)))
        self.test_initialization = bool(kw.get("test_initialization", g("test_initialization", True)))
        self.test_compute_loss = bool(kw.get("test_compute_loss", g("test_compute_loss", False)))
        if any(v <= 0 for v in self.test_iter):
            raise ValueError("test_iter: every entry must be positive")
        has_net = g("net") is not None or "net" in kw
        generic = len(self.test_iter) - len(self.test_net) if has_net else 0
        if len(self.test_net) > len(self.test_iter):
            raise ValueError("test_iter: %d given for %d test_net files (one test_iter per test net)" % (len(self.test_iter), len(self.test_net)))
        if len(self.test_net) + generic != len(self.test_iter):
            raise ValueError("test_iter: %d given but only %d test nets (test_net files, plus `net` in TEST phase)" % (
                len(self.test_iter), len(self.test_net) + generic))
        net = kw.get("net", g("net"))
        # [(file, test_iter)]: what Solver builds, in Caffe's order
        self.test_instances: List[Tuple[str, int]] = list(zip(self.test_net + [str(net)] * generic, self.test_iter))
        if self.test_instances and self.test_interval <= 0:
            raise ValueError("test_interval: must be > 0 when a test net is given (%d)" % self.test_interval)
        if self.test_interval < 0:
            raise ValueError("test_interval: %d is negative" % self.test_interval)

    @property
    def histories(self) -> int:
        """History buffers per learnable blob (what a .solverstate of this type carries per blob)."""
        return 2 if self.kind in ("ADAM", "ADADELTA") else 1

    def test_due(self, it: int) -> bool:
        """Solver::Step's test condition at the top of iteration `it`."""
        return self.test_interval > 0 and it % self.test_interval == 0 and (it > 0 or self.test_initialization)

    def rate(self, it: int) -> float:
        """SGDSolver::GetLearningRate; multistep counts the stepvalues passed instead of carrying current_step, so a resumed run
        needs no extra state."""
        p, b = self.lr_policy, self.base_lr
        if p == "fixed":
            return b
        if p == "step":
            return b * self.gamma ** (it // self.stepsize)
        if p == "exp":
            return b * self.gamma ** it
        if p == "inv":
            return b * (1.0 + self.gamma * it) ** (-self.power)
        if p == "multistep":
            return b * self.gamma ** sum(1 for v in self.stepvalue if v <= it)
        if p == "poly":
            return b * (1.0 - float(it) / self.max_iter) ** self.power
        return b / (1.0 + math.exp(-self.gamma * (it - self.stepsize)))


class TrainEngine(Engine):
    """Engine for the TRAIN phase with backward pass and solver state."""

    def __init__(self, spec: NetSpec, data_shapes: Dict[str, Tuple[int, ...]], params=None, device: int = 0,
                 solver: Optional[SolverParams] = None, comm=None, autotune: bool = True):
        super().__init__(spec, data_shapes, params, device, fuse=True, group_convs=True, autotune=autotune, solver=solver, comm=comm)
        self._alloc_solver_state()
        self._build_backward()

    def _init_state(self, spec: NetSpec, data_shapes=None, *, solver: Optional[SolverParams] = None, comm=None, **kw) -> None:
        """Engine._init_state plus the training state: the solver, the gradient blobs and the backward plan's slots (_adopt_backward fills them)."""
        if spec.phase != "TRAIN":
            raise ValueError("TrainEngine needs a TRAIN-phase NetSpec")
        self.solver = solver or SolverParams()
        self.comm = comm                      # None or an object with all_reduce_sum(ptr, count, stream) and .world
        self.grad_blobs: Dict[str, Blob] = {}
        self.bwd_ops: List[Op] = []
        self.iter = 0
        self._ws = self._ip_ws = self._ip_wgrad_ws = self._gate_ws = self._act_ws = None
        self._flip_flat = self._flip_segs_dev = self._tbank = None
        super()._init_state(spec, data_shapes, **kw)

    # ------------------------------------------------------------------ gradient buffers
    def _learns(self, l: Layer) -> bool:
        """True if the solver will move any blob of this layer: Caffe's param_propagate_down (lr_mult != 0)."""
        if l.name not in self.spec.param_shapes or l.type == "BatchNorm":      # (BatchNorm's blobs are statistics: lr_mult 0, forced)
            return False
        n = len(self.spec.param_shapes[l.name])
        return any((l.lr_mult[i] if i < len(l.lr_mult) else 1.0) != 0.0 for i in range(n))

    def _needs_grad(self) -> set:
        """Blobs downstream of a layer that learns (Caffe's propagate_down): only those carry gradients.  Frozen layers
        (lr_mult 0: conv1_1..conv3_3 of train/bounding_box, every bilinear deconvolution) neither get a weight gradient
        nor pull the backward pass below them."""
        need = set()
        for l in self.spec.layers:
            if l.type in DATA_TYPES:
                continue
            through = l.bottoms[:1] if l.type in ("Crop", "Upsample") else l.bottoms      # a Crop's second bottom only lends its shape, an Upsample's is the mask
            if self._learns(l) or any(b in need for b in through):
                need.update(l.tops)
        return need

    def _plan_buffers(self) -> None:
        super()._plan_buffers()
        need = self._needs_grad()
        self.need_grad = need
        roots: Dict[int, DeviceBuffer] = {}      # activation buffer address -> gradient buffer
        for name, b in self.blobs.items():
            if name not in need or b.nchw is None:
                continue
            gb = roots.get(b.buf.ptr)
            if gb is None:
                gb = DeviceBuffer(b.buf.nbytes, zero=True)
                roots[b.buf.ptr] = gb
            g = Blob(name, b.shape)
            g.rows = b.rows
            g.buf, g.coffset, g.cstride = gb, b.coffset, b.cstride
            self.grad_blobs[name] = g

    def _loss_grad_ptr(self, blob: str) -> Optional[int]:
        g = self.grad_blobs.get(blob)
        if g is None:
            return None
        if g.coffset:
            raise NotImplementedError("loss gradient into a channel slice")
        return g.ptr

    # ------------------------------------------------------------------ solver state
    def _alloc_solver_state(self) -> None:
        n = max(self.param_count, 4)
        self.grad_flat = DeviceBuffer(n * 4, zero=True)
        self.hist = DeviceBuffer(n * 4, zero=True)
        self.hist2 = DeviceBuffer(n * 4, zero=True) if self.solver.histories == 2 else None
        # iter_size > 1: every pass overwrites grad_flat; fcn_grad_accumulate_f32 sums the passes here, and the update reads this
        self.acc_flat = DeviceBuffer(n * 4, zero=True) if self.solver.iter_size > 1 else None
        self._pass = 0
        self._pass_losses: List[Dict[str, float]] = []
        # clip_gradients: the factor is computed and consumed on the device (no read-back inside a step)
        self.clip_dev = self.clip_ws = None
        if self.solver.clip_gradients > 0:
            self.clip_dev = DeviceBuffer(16, zero=True)      # word 0: the factor, word 1: the sum of squares (for read_clip())
            self.clip_ws = DeviceBuffer(int(L.load().fcn_grad_clip_workspace_bytes()), zero=False)
        segs = (L.SolverSeg * len(self.param_layout))(*[
            L.SolverSeg(e.offset, e.count, e.lr_mult, e.decay_mult) for e in self.param_layout])
        self._segs_host = segs
        self.segs_dev = DeviceBuffer(max(C.sizeof(segs), 16), zero=False)
        L.call("fcn_memcpy_h2d_async", self.segs_dev.ptr, C.addressof(segs), C.sizeof(segs), None)
        L.call("fcn_device_sync")
        # pinned: the loss read-back at the end of step_begin() must not hold the host thread until the step has run (a
        # pageable destination makes the "async" copy synchronous, and the next batch could not be prepared meanwhile)
        self._loss_pinned = {name: PinnedArray((1,)) for name in self.loss_blobs}
        self.loss_host = {name: p.array for name, p in self._loss_pinned.items()}

    def _grad_view(self, layer: str, index: int) -> DevView:
        seg = self.param_segs[(layer, index)]
        return DevView(self.grad_flat.ptr + 4 * seg.offset, 4 * seg.count)

    # ------------------------------------------------------------------ backward plan
    def _build_backward(self) -> None:
        plan = BackwardPlanner(self)
        plan.run()
        self._adopt_backward(plan)
        if self.autotune:
            self.tuner.wgrad_cfgs(self.bwd_ops)
        self.tuner.release()
        self._plan_buckets()

    def _adopt_backward(self, plan: BackwardPlanner) -> None:
        """Take the launches and the workspaces of a finished backward plan."""
        self.bwd_ops, self._ws, self._ip_ws, self._ip_wgrad_ws = plan.ops, plan.ws, plan.ip_ws, plan.ip_wgrad_ws
        self._gate_ws = plan.gate_ws      # the gate gradients of the gated Scale layers (backward._scale_gate); None without one
        self._act_ws = plan.act_ws        # the parameter gradients of PReLU and Bias layers (backward._act); None without one
        self._flip_flat, self._flip_segs_dev, self._tbank = plan.flip_flat, plan.flip_segs_dev, plan.tbank

    def _plan_buckets(self, bucket_floats: int = 1536 * 1024) -> None:
        """Gradient buckets for the overlapped all-reduce: contiguous ranges of the flat gradient buffer (forward layer
        order).  Backward fills the buffer roughly from its end; a bucket is complete once the LAST of its layers' weight
        gradient launches (grouped launches reorder them within a module) has been enqueued; its all-reduce then runs on a
        side stream while the main stream continues with earlier layers."""
        self.buckets: List[dict] = []
        if self.comm is None:
            return
        cur = None
        for e in self.param_layout:
            if cur is None or (e.index == 0 and cur["count"] >= bucket_floats):
                cur = dict(offset=e.offset, count=0, layers=[])
                self.buckets.append(cur)
            cur["count"] = e.offset + _r4(e.count) - cur["offset"]
            if e.layer not in cur["layers"]:
                cur["layers"].append(e.layer)
        wg_index = {}
        for i, op in enumerate(self.bwd_ops):
            if op.kind == "wgrad" or hasattr(op, "layers"):      # (a main-stream launch that writes parameter gradients names its layers too)
                for nm in getattr(op, "layers", [op.name]):
                    wg_index[nm] = i
        lib = L.load()
        sp = C.c_void_p()
        L.call("fcn_stream_create", C.byref(sp))
        self.comm_stream = int(sp.value)
        for b in self.buckets:
            done = [wg_index[nm] for nm in b["layers"] if nm in wg_index]
            b["after_op"] = max(done) if done else len(self.bwd_ops) - 1
            for key in ("ready", "done"):
                ev = C.c_void_p()
                L.call("fcn_event_create", C.byref(ev))
                b[key] = ev

    def _fused_relu_layers(self) -> set:
        if not hasattr(self, "_fused_relu_cache"):
            out = set()
            layers = self.spec.layers
            for li, l in enumerate(layers):
                if l.type in ("Convolution", "DepthwiseConvolution", "InnerProduct") and self._conv_layer_meta.get(l.name, {}).get("relu"):
                    top = l.tops[0]
                    for nxt in layers[li + 1:]:
                        if top in nxt.bottoms or top in nxt.tops:
                            if nxt.type == "ReLU":
                                out.add(nxt.name)
                            break
            out.update(ch.relu.name for ch in self._bn_chains.values() if ch.relu is not None)      # ... or into a BatchNorm / Scale chain
            self._fused_relu_cache = out
        return self._fused_relu_cache

    # ------------------------------------------------------------------ one solver iteration
    def step(self, seed: Optional[int] = None, upload: bool = True, feed: Optional[Callable[[int], None]] = None) -> Dict[str, float]:
        """Solver::Step for one iteration.  Inputs come from the input blobs' host arrays (upload=True), except label
        blobs staged with set_targets(), which are generated on the device; upload=False reuses what is already in HBM.
        Returns {loss blob: value} plus 'total_loss' = sum of loss_weight * value (what `caffe train` prints; also under
        'loss' when no blob has that name).
        With iter_size k > 1 the iteration is k forward / backward passes whose gradients are summed before one update;
        feed(j), when given, is called before pass j to put that pass's batch into the host arrays (without it every pass sees
        what the caller filled in).  The losses returned are the means over the passes."""
        out: Dict[str, float] = {}
        for j in range(self.solver.iter_size):
            if feed is not None:
                feed(j)
            self.step_begin(seed, upload)
            out = self.step_end()
        return out

    def step_begin(self, seed: Optional[int] = None, upload: bool = True) -> None:
        """Enqueue a whole iteration (inputs, targets, forward, backward, all-reduce, update, loss read-back) and return
        without waiting: the caller may prepare the next batch while the device works (step_end() collects the losses).
        With iter_size k > 1 one call is one of the k passes of the iteration: forward, backward and the accumulation of its
        gradients; the last pass adds the all-reduce of the accumulated buffer, clipping and the update."""
        lib = L.load()
        with self.lock:
            L.call("fcn_init", self.device)
            k = self.solver.iter_size
            last = self._pass == k - 1
            self.dropout_seed = int(seed if seed is not None else self.iter * k + self._pass) & 0xFFFFFFFF
            dev_targets = getattr(self, "_tgt", None) is not None and self._tgt.get("pending")
            fed = set(self.device_fed)      # inputs some producer already wrote in HBM (device scene renderer)
            if upload:
                skip = (set(self._tgt["tops"]) if dev_targets else set()) | fed
                for nm in self.inputs:
                    if nm not in skip:
                        self._enqueue_upload(nm, self.stream)
            if dev_targets:
                self._enqueue_targets()
            world = self.comm.world if self.comm is not None else 1
            side = self._wgrad_stream()
            side_used = False
            for kind, item in self._step_plan():
                if kind == "graph":
                    L.check(lib.fcn_graph_launch(item, self.stream))
                elif kind == "op":
                    item.run(self.stream)
                elif kind == "fork":
                    op, ev0, ev1 = item
                    L.check(lib.fcn_event_record(ev0, self.stream))
                    L.check(lib.fcn_stream_wait_event(side, ev0))
                    op.run(side)
                    L.check(lib.fcn_event_record(ev1, side))
                elif kind == "join":
                    L.check(lib.fcn_stream_wait_event(self.stream, item))
                elif kind == "side":
                    # a weight gradient: nothing later in this step reads it except the update, and its inputs (dY, X) are
                    # final here -> it runs on the second stream beside the data-gradient chain
                    op, ev = item
                    L.check(lib.fcn_event_record(ev, self.stream))
                    L.check(lib.fcn_stream_wait_event(side, ev))
                    op.run(side)
                    side_used = True
                elif k > 1:
                    continue        # (the ranks exchange the ACCUMULATED buffer, once, after the last pass)
                else:
                    for b in item:
                        # this bucket's gradients are final: sum them across ranks on the side stream
                        if side_used:       # final = everything queued so far on BOTH streams
                            if "ready_main" not in b:
                                ev = C.c_void_p()
                                L.call("fcn_event_create", C.byref(ev))
                                b["ready_main"] = ev
                            L.check(lib.fcn_event_record(b["ready_main"], self.stream))
                            L.check(lib.fcn_stream_wait_event(side, b["ready_main"]))
                        L.check(lib.fcn_event_record(b["ready"], side if side_used else self.stream))
                        L.check(lib.fcn_stream_wait_event(self.comm_stream, b["ready"]))
                        if not getattr(self, "comm_dry", False):      # (benchmarks: the same step without the collective)
                            if getattr(self, "_replicas_diverged", False):
                                raise RuntimeError("TrainEngine: a comm_dry step applied un-reduced gradients; the replicas no longer hold the "
                                                   "same weights and this engine must not take real data-parallel steps (bench.py closes it)")
                            self.comm.all_reduce_sum(self.grad_flat.ptr + 4 * b["offset"], b["count"], self.comm_stream)
                        elif world > 1:
                            self._replicas_diverged = True
                        L.check(lib.fcn_event_record(b["done"], self.comm_stream))
            if k == 1:
                for b in self.buckets:
                    L.check(lib.fcn_stream_wait_event(self.stream, b["done"]))
            if side_used:
                L.check(lib.fcn_event_record(self._side_done, side))
                L.check(lib.fcn_stream_wait_event(self.stream, self._side_done))
            if k > 1:
                L.check(lib.fcn_grad_accumulate_f32(self.acc_flat.ptr, self.grad_flat.ptr, max(self.param_count, 4), int(self._pass == 0),
                                                    self.stream))
                if last and self.comm is not None and world > 1:
                    if getattr(self, "comm_dry", False):
                        self._replicas_diverged = True
                    else:
                        self.comm.all_reduce_sum(self.acc_flat.ptr, max(self.param_count, 4), self.stream)
            if last:
                self.apply_update(1.0 / (world * k), 1.0 / world)
            for name, arr in self.loss_host.items():
                L.check(lib.fcn_memcpy_d2h_async(arr.ctypes.data, self.blobs[name].buf.ptr, 4, self.stream))
            if getattr(self, "_step_done", None) is None:
                ev = C.c_void_p()
                L.call("fcn_event_create", C.byref(ev))
                self._step_done = ev
            L.check(lib.fcn_event_record(self._step_done, self.stream))
            self._in_flight = (list(self._tgt["tops"]) if dev_targets else []) + list(fed)

    def time_allreduce(self, reps: int = 10) -> Dict[str, float]:
        """The step's gradient all-reduce alone: every bucket back to back on the communication stream, nothing else on
        the GPU (every rank must call this together).  Returns microseconds per full-gradient all-reduce, the bytes summed
        and the bus bandwidth 2 (G-1)/G * bytes / time of the usual collective accounting."""
        if self.comm is None or not self.buckets:
            return {"allreduce_us": 0.0, "bytes": 0, "bus_GBps": 0.0, "buckets": 0}
        with self.lock:
            L.call("fcn_device_sync")
            e0, e1 = C.c_void_p(), C.c_void_p()
            L.call("fcn_event_create", C.byref(e0))
            L.call("fcn_event_create", C.byref(e1))
            scratch = DeviceBuffer(self.grad_flat.nbytes)      # summing zeros: the gradients themselves stay untouched
            for r in range(reps + 2):
                if r == 2:
                    L.call("fcn_event_record", e0, self.comm_stream)
                for b in self.buckets:
                    self.comm.all_reduce_sum(scratch.ptr + 4 * b["offset"], b["count"], self.comm_stream)
            L.call("fcn_event_record", e1, self.comm_stream)
            L.call("fcn_event_sync", e1)
            ms = C.c_float()
            L.call("fcn_event_elapsed_ms", e0, e1, C.byref(ms))
            L.call("fcn_event_destroy", e0)
            L.call("fcn_event_destroy", e1)
            scratch.free()
        nbytes = 4 * sum(b["count"] for b in self.buckets)
        us = ms.value * 1e3 / reps
        g = self.comm.world
        return {"allreduce_us": us, "bytes": nbytes, "buckets": len(self.buckets),
                "bus_GBps": (2.0 * (g - 1) / g * nbytes / (us * 1e-6) / 1e9) if us > 0 else 0.0}

    def step_end(self) -> Dict[str, float]:
        with self.lock:
            L.call("fcn_event_sync", self._step_done)
            for b in self.blobs.values():
                b.host_valid = b.is_input
            for nm in self._in_flight:
                self.blobs[nm].host_valid = False          # generated in HBM, never on the host
            out = {k: float(v[0]) for k, v in self.loss_host.items()}
            if self.solver.iter_size > 1:
                # one pass of an accumulated iteration: what is displayed and averaged is the mean over its passes, and the
                # iteration counter moves with the update, after the last of them
                self._pass_losses.append(out)
                out = {k: float(sum(p[k] for p in self._pass_losses) / len(self._pass_losses)) for k in out}
                self._pass += 1
                if self._pass == self.solver.iter_size:
                    self._pass, self._pass_losses = 0, []
                    self.iter += 1
            else:
                self.iter += 1
            out["total_loss"] = float(sum(self.loss_blobs[k] * out[k] for k in self.loss_blobs))
            out.setdefault("loss", out["total_loss"])      # shorthand, unless a blob is itself called "loss" (train/fcn_bbox)
            return out

    # kinds whose launch arguments change from step to step (the dropout seed): they stay ordinary launches
    DYNAMIC_KINDS = ("dropout", "dropout_bwd")

    def _wgrad_stream(self) -> Optional[int]:
        """Second stream for the weight-gradient launches (FCN_WGRAD_STREAM=0 keeps everything on one stream)."""
        import os
        if os.environ.get("FCN_WGRAD_STREAM", "1") == "0":
            return None
        if getattr(self, "_side_stream", None) is None:
            sp, ev = C.c_void_p(), C.c_void_p()
            L.call("fcn_stream_create", C.byref(sp))
            L.call("fcn_event_create", C.byref(ev))
            self._side_stream, self._side_done = int(sp.value), ev
        return self._side_stream

    def _step_plan(self) -> List[Tuple[str, object]]:
        """Forward + backward of one step as [("graph", hipGraphExec) | ("op", Op) | ("reduce", [buckets])].
        Maximal runs of launches with step-invariant arguments are captured once into hipGraphs (a step is ~240
        launches, most of them a few microseconds long: inside a graph the gap between two of them is about half of
        what a stream launch costs); dropout and the points where a gradient bucket goes to RCCL stay outside."""
        if getattr(self, "_plan", None) is not None:
            return self._plan
        import os
        # the first step runs as ordinary launches (code objects load lazily on a kernel's first launch, which must not
        # happen inside a stream capture); graphs are captured from the second step on
        first = not getattr(self, "_warm", False)
        self._warm = True
        use_graph = os.environ.get("FCN_TRAIN_GRAPH", "1") != "0" and graphs_enabled() and not first
        triggers: Dict[int, List[dict]] = {}
        for b in self.buckets:
            triggers.setdefault(b["after_op"], []).append(b)
        seq: List[Tuple[str, object]] = [("op", op) for op in self.ops]
        for i, op in enumerate(self.bwd_ops):
            seq.append(("op", op))
            if i in triggers:
                seq.append(("reduce", triggers[i]))
        plan: List[Tuple[str, object]] = []
        run: List[Op] = []

        def flush() -> None:
            if not run:
                return
            if use_graph and len(run) > 1:
                L.call("fcn_graph_begin", self.stream)
                try:
                    for op in run:
                        op.run(self.stream)
                finally:
                    g = C.c_void_p()
                    L.call("fcn_graph_end", self.stream, C.byref(g))
                self._step_graphs.append(int(g.value))
                plan.append(("graph", int(g.value)))
            else:
                plan.extend(("op", op) for op in run)
            run.clear()

        self._step_graphs: List[int] = getattr(self, "_step_graphs", [])
        side = self._wgrad_stream() is not None

        def new_event():
            ev = C.c_void_p()
            L.call("fcn_event_create", C.byref(ev))
            self._keep.append(ev)
            return ev
        if side and self.bwd_ops and self.bwd_ops[0].kind == "flip":
            # the flipped filter banks depend on the weights only: refreshed beside the forward pass, joined before backward
            at = len(self.ops)
            flip_evs = (new_event(), new_event())
            seq[at] = ("join", flip_evs[1])
            seq.insert(0, ("fork", (self.bwd_ops[0], flip_evs[0], flip_evs[1])))
        for kind, item in seq:
            if kind == "op" and side and item.kind == "wgrad":
                flush()
                plan.append(("side", (item, new_event())))
                continue
            if kind == "op" and item.kind not in self.DYNAMIC_KINDS:
                run.append(item)
                continue
            flush()
            plan.append((kind, item))
        flush()
        if not first:
            self._plan = plan
        return plan

    def close(self) -> None:
        lib = L.load()
        for g in getattr(self, "_step_graphs", []):
            lib.fcn_graph_destroy(g)
        self._step_graphs = []
        self._plan = None
        if getattr(self, "_side_stream", None):
            lib.fcn_stream_sync(self._side_stream)
            lib.fcn_stream_destroy(self._side_stream)
            self._side_stream = None
        super().close()

    def apply_update(self, grad_scale: float, norm_scale: float = 1.0) -> None:
        """ClipGradients + Normalize + Regularize + ComputeUpdateValue + Update of Caffe's solvers on the flat buffers.
        grad_scale: 1 / (ranks * iter_size); norm_scale: 1 / ranks (clipping sees the gradient summed over iter_size, averaged
        over the ranks).  SGD and Adam with L2 and without clipping take the two original entry points."""
        sp, lib = self.solver, L.load()
        rate = sp.rate(self.iter)
        n = len(self.param_layout)
        g = self.acc_flat if self.acc_flat is not None else self.grad_flat
        l1 = sp.regularization_type == "L1"
        clip = None
        if self.clip_dev is not None:
            clip = self.clip_dev.ptr
            L.check(lib.fcn_grad_clip_f32(g.ptr, self.segs_dev.ptr, n, sp.clip_gradients, norm_scale, clip, clip + 4, self.clip_ws.ptr,
                                          self.stream))
        if sp.kind == "ADAM" and not l1 and clip is None:
            L.check(lib.fcn_adam_update_f32(self.param_flat.ptr, g.ptr, self.hist.ptr, self.hist2.ptr, self.segs_dev.ptr, n, rate,
                                            sp.momentum, sp.momentum2, sp.delta, sp.weight_decay, self.iter + 1, grad_scale, self.stream))
        elif sp.kind == "SGD" and not l1 and clip is None:
            L.check(lib.fcn_sgd_update_f32(self.param_flat.ptr, g.ptr, self.hist.ptr, self.segs_dev.ptr, n, rate, sp.momentum,
                                           sp.weight_decay, grad_scale, self.stream))
        else:
            L.check(lib.fcn_solver_update_f32(L.SOLVER_KINDS[sp.kind], self.param_flat.ptr, g.ptr, self.hist.ptr,
                                              self.hist2.ptr if self.hist2 is not None else None, self.segs_dev.ptr, n, rate, sp.momentum,
                                              sp.momentum2, sp.rms_decay, sp.delta, sp.weight_decay, L.REG_L1 if l1 else L.REG_L2,
                                              self.iter + 1, grad_scale, clip, self.stream))

    def read_clip(self) -> Tuple[float, float]:
        """(clip factor, sum of squares of the gradient) of the last update, or (1.0, nan) when clip_gradients is off (debug / tests)."""
        if self.clip_dev is None:
            return 1.0, float("nan")
        out = np.empty(2, F32)
        L.call("fcn_memcpy_d2h_async", out.ctypes.data, self.clip_dev.ptr, out.nbytes, self.stream)
        L.call("fcn_stream_sync", self.stream)
        return float(out[0]), float(out[1])

    # ------------------------------------------------------------------ parameters back to Caffe layout
    def download_params(self) -> Dict[str, List[np.ndarray]]:
        """Current parameters as Caffe-layout host arrays (conv: OIHW, bias)."""
        flat = np.empty(max(self.param_count, 4), F32)
        L.call("fcn_memcpy_d2h_async", flat.ctypes.data, self.param_flat.ptr, flat.nbytes, self.stream)
        L.call("fcn_stream_sync", self.stream)
        return self._unpack(flat)

    def download_grads(self) -> Dict[str, List[np.ndarray]]:
        """Parameter gradients of the last iteration: with iter_size > 1 their sum over its passes (not divided by iter_size)."""
        flat = np.empty(max(self.param_count, 4), F32)
        src = self.acc_flat if self.acc_flat is not None else self.grad_flat
        L.call("fcn_memcpy_d2h_async", flat.ctypes.data, src.ptr, flat.nbytes, self.stream)
        L.call("fcn_stream_sync", self.stream)
        return self._unpack(flat)

    def _unpack(self, flat: np.ndarray) -> Dict[str, List[np.ndarray]]:
        out: Dict[str, List[np.ndarray]] = {}
        for e in self.param_layout:
            out.setdefault(e.layer, []).append(S.unpack(e, flat[e.offset:e.offset + e.count]))
        return out

    def _pack(self, per_layer: Dict[str, List[np.ndarray]]) -> np.ndarray:
        """Inverse of _unpack: Caffe-layout blobs -> the flat device layout (padded input channels stay zero)."""
        flat = np.zeros(max(self.param_count, 4), F32)
        for e in self.param_layout:
            flat[e.offset:e.offset + e.count] = S.pack(e, per_layer[e.layer][e.index]).reshape(-1)
        return flat

    def download_history(self) -> List[np.ndarray]:
        """Solver history in Caffe's order: one blob per learnable parameter (SGD / Nesterov momentum, the AdaGrad / RMSProp sums,
        Adam's m, AdaDelta's gradient history), then for Adam and AdaDelta as many again (v / the update history)."""
        out: List[np.ndarray] = []
        for buf in (self.hist, self.hist2):
            if buf is None:
                continue
            flat = np.empty(max(self.param_count, 4), F32)
            L.call("fcn_memcpy_d2h_async", flat.ctypes.data, buf.ptr, flat.nbytes, self.stream)
            L.call("fcn_stream_sync", self.stream)
            per = self._unpack(flat)
            for l in self.spec.param_layers():
                out.extend(per[l.name])
        return out

    def upload_history(self, history: Sequence[np.ndarray]) -> None:
        bufs = [b for b in (self.hist, self.hist2) if b is not None]
        per_buf = sum(len(self.params_host[l.name]) for l in self.spec.param_layers())
        if len(history) != per_buf * len(bufs):
            raise ValueError("solver state holds %d history blobs, a %s solver over this net needs %d" % (
                len(history), self.solver.kind, per_buf * len(bufs)))
        k = 0
        for _ in bufs:
            for l in self.spec.param_layers():
                for a in self.params_host[l.name]:
                    if np.asarray(history[k]).size != a.size:
                        raise ValueError("solver state: history blob %d has %d values, blob of layer %s has %d" % (
                            k, np.asarray(history[k]).size, l.name, a.size))
                    k += 1
        it = iter(history)
        for buf in bufs:
            per = {l.name: [next(it) for _ in self.params_host[l.name]] for l in self.spec.param_layers()}
            flat = self._pack(per)
            L.call("fcn_memcpy_h2d_async", buf.ptr, flat.ctypes.data, flat.nbytes, self.stream)
            L.call("fcn_stream_sync", self.stream)

    def read_grad(self, name: str) -> np.ndarray:
        """NCHW host copy of a blob's gradient (debug / tests)."""
        g = self.grad_blobs[name]
        n, c, h, w = g.nchw
        raw = np.empty((n, h, w, g.cstride), F32)
        L.call("fcn_memcpy_d2h_async", raw.ctypes.data, g.buf.ptr, raw.nbytes, self.stream)
        L.call("fcn_stream_sync", self.stream)
        return np.ascontiguousarray(raw[..., g.coffset:g.coffset + c].transpose(0, 3, 1, 2)).reshape(g.shape)

    def save(self, path: str) -> None:
        params = self.download_params()
        layers = [(l.name, l.type, params[l.name]) for l in self.spec.param_layers()]
        proto.write_caffemodel(path, layers, self.spec.name)
