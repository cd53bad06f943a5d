"""Device executor: turns a :class:`NetSpec` into a launch plan over libfcnhip.so.

This is the MI355X replacement of the tensor engine the reference reaches
through ``caffe.Net`` (reference: scripts/fcn_object_detector.py:87,317-328).

Design:
  * activations live in HBM as NHWC float32 with a per-blob channel stride;
    Concat is free — the producers of an inception module write their channel
    slice of the concat buffer directly;
  * ReLU (in place after a conv), the Sigmoid coverage head and the Power(shift)
    input transform are fused into the convolution kernel's prologue/epilogue;
  * layers are scheduled by dependency level and all convolutions of one level
    (inception branches, the two heads) share ONE grouped launch;
  * the whole forward is captured once into a hipGraph and replayed per frame,
    so the per-frame host cost is one graph launch.
Blob contents are exposed to Python as NCHW float32 (pycaffe layout); the
NCHW<->NHWC change happens on the device at the boundary only.
"""
from __future__ import annotations

import ctypes as C
import os
import threading
from collections import namedtuple
from dataclasses import dataclass, field
from typing import Callable, Dict, List, Optional, Sequence, Tuple, Union

import numpy as np

from . import lib as L
from . import region as RG
from . import ssd as SSD
from . import storage as S
from . import tune as T
from .netspec import (ACT_TYPES, NEURON_TYPES, SHUFFLE_TYPES, Layer, NetSpec, argmax_form, bn_global_stats, crop_window, interp_size, is_rectangular, is_scale_gate, kernel_stride_pad,
                      layer_dilation, layer_geometry, neuron_params, scale_gate_form, shuffle_group)
from .storage import _r4, _ra, ip_pack_bank, ip_unpack_bank      # noqa: F401  (the bank helpers stay importable from here)

F32 = np.float32


def graphs_enabled() -> bool:
    """False under FCN_NO_GRAPH=1: plain launches instead of hipGraphs (e.g. under a profiler).  Reads the environment at every
    call - tests and tools set the variable after import."""
    return os.environ.get("FCN_NO_GRAPH", "0") in ("", "0")


_replica_ctx = threading.local()


class replica_streams:
    """Context under which every Engine built (by this thread) is a replica of a frame pipeline and takes a replica stream
    (fcn_stream_create_replica: a hardware queue that the null stream and the process's plain streams do not share), numbered
    in the order of construction.  For pipelines whose engines come from a caller's factory (DetectorPipeline); lone engines and
    the training engine's streams stay plain."""

    def __enter__(self) -> "replica_streams":
        self._outer = getattr(_replica_ctx, "next", None)
        _replica_ctx.next = 0
        return self

    def __exit__(self, *exc) -> None:
        _replica_ctx.next = self._outer


def _take_replica_index() -> Optional[int]:
    i = getattr(_replica_ctx, "next", None)
    if i is not None:
        _replica_ctx.next = i + 1
    return i


def dropout_layer_salt(spec: NetSpec, l: Layer) -> int:
    """What the k-th Dropout layer of a net adds to the step's dropout seed: k * 2^28.  The mask is a function of (element index, seed)
    alone, so two Dropout layers of one shape (drop6 / drop7 of the published FCN nets) would otherwise drop the same units in every
    step.  0 for the first layer: nets with one Dropout layer draw what they always drew.  Seeds count iterations, so layer k at
    iteration i draws what layer 0 draws at iteration i + k * 2^28 - beyond any run."""
    k = [q.name for q in spec.layers if q.type == "Dropout"].index(l.name)
    return (k << 28) & 0xFFFFFFFF


class ConvGeom(namedtuple("ConvGeom", "n cin h w cout oh ow k s pad")):
    """The convolution-shaped geometry of one layer (Convolution, Deconvolution, Pooling): input n x cin x h x w, output
    n x cout x oh x ow, square kernel k at stride s with padding pad."""
    __slots__ = ()

    @property
    def flops(self) -> float:
        return 2.0 * self.n * self.cout * self.oh * self.ow * self.cin * self.k * self.k

    def swapped(self) -> "ConvGeom":
        """The same layer seen from its output: input and output trade places (data-gradient passes, Deconvolution backward)."""
        return self._replace(cin=self.cout, h=self.oh, w=self.ow, cout=self.cin, oh=self.h, ow=self.w)


def conv_desc(x: "Blob", y: "Blob", g: ConvGeom, w: Optional[int] = None, bias: Optional[int] = None, flags: int = 0) -> L.ConvDesc:
    """fcn_conv_desc of the problem `g` as the kernel sees it (the caller has rounded Cin and swapped roles where it must) reading
    the view x and writing the view y - activations or gradients."""
    d = L.ConvDesc()
    d.x, d.w, d.bias, d.y = x.ptr, w, bias, y.buf.ptr
    d.N, d.H, d.W, d.Cin, d.x_cstride = g.n, g.h, g.w, g.cin, x.cstride
    d.Cout, d.kh, d.kw, d.pad, d.stride, d.OH, d.OW = g.cout, g.k, g.k, g.pad, g.s, g.oh, g.ow
    d.y_cstride, d.y_coffset = y.cstride, y.coffset
    d.flags = flags
    return d


def tconv_desc(a: "Blob", b: "Blob", g: ConvGeom, bank: int, bias: Optional[int] = None, flags: int = 0) -> L.TConvDesc:
    """fcn_tconv_desc: the transposed convolution that reads the view a (n x cin x h x w of g) through the tap-major bank and
    writes the view b (n x cout x oh x ow)."""
    d = L.TConvDesc()
    d.a, d.w, d.bias, d.b = a.ptr, bank, bias, b.buf.ptr
    d.N, d.H, d.W, d.Ca, d.a_cstride = g.n, g.h, g.w, g.cin, a.cstride
    d.Cb, d.kh, d.kw, d.pad, d.stride, d.OH, d.OW = g.cout, g.k, g.k, g.pad, g.s, g.oh, g.ow
    d.b_cstride, d.b_coffset = b.cstride, b.coffset
    d.flags = flags
    return d


class RectGeom(namedtuple("RectGeom", "n cin h w cout oh ow kh kw sh sw ph pw d")):
    """The geometry of a rectangular or dilated Convolution (csrc/rconv.hip): input n x cin x h x w, output n x cout x oh x ow, kernel
    kh x kw at strides (sh, sw) with pads (ph, pw) and one dilation d for both axes.  A square dilated layer has equal axes."""
    __slots__ = ()

    @property
    def flops(self) -> float:
        return 2.0 * self.n * self.oh * self.ow * self.cin * self.cout * self.kh * self.kw

    @property
    def bytes(self) -> float:
        return 4.0 * (self.n * self.cin * self.h * self.w + self.n * self.cout * self.oh * self.ow + self.cout * self.cin * self.kh * self.kw + self.cout)

    def bytes_as(self, xsize: int, ysize: int) -> float:
        """`bytes` with x and the bank in elements of xsize bytes, y in elements of ysize bytes (the bias stays float32)."""
        return float(xsize * (self.n * self.cin * self.h * self.w + self.cout * self.cin * self.kh * self.kw) +
                     ysize * self.n * self.cout * self.oh * self.ow + 4 * self.cout)

    def swapped(self) -> "RectGeom":
        """The same layer seen from its output: input and output trade places (the data-gradient pass)."""
        return self._replace(cin=self.cout, h=self.oh, w=self.ow, cout=self.cin, oh=self.h, ow=self.w)


def rconv_desc(x: "Blob", y: "Blob", g: RectGeom, w: Optional[int] = None, bias: Optional[int] = None, flags: int = 0) -> L.RConvDesc:
    """fcn_rconv_desc: the rectangular or dilated convolution `g` reading the view x through the OHWI bank w and writing the view y - activations
    (forward) or gradients (the data-gradient pass on the flipped bank, the weight gradient with y = dY)."""
    d = L.RConvDesc()
    d.x, d.w, d.bias, d.y = x.ptr, w, bias, y.buf.ptr
    d.N, d.H, d.W, d.Cin, d.x_cstride = g.n, g.h, g.w, g.cin, x.cstride
    d.Cout, d.kh, d.kw, d.pad_h, d.pad_w, d.stride_h, d.stride_w, d.OH, d.OW = g.cout, g.kh, g.kw, g.ph, g.pw, g.sh, g.sw, g.oh, g.ow
    d.y_cstride, d.y_coffset = y.cstride, y.coffset
    d.flags, d.dilation = flags, g.d
    return d


class DwGeom(namedtuple("DwGeom", "n c h w oh ow kh kw sh sw ph pw d")):
    """The geometry of a depthwise Convolution (csrc/dwconv.hip): n x c x h x w in, n x c x oh x ow out, kernel kh x kw at strides
    (sh, sw) with pads (ph, pw) and one dilation d for both axes."""
    __slots__ = ()

    @property
    def flops(self) -> float:
        return 2.0 * self.n * self.oh * self.ow * self.c * self.kh * self.kw

    @property
    def bytes(self) -> float:
        return 4.0 * (self.n * self.h * self.w * self.c + self.n * self.oh * self.ow * self.c + self.kh * self.kw * self.c + self.c)


def dwconv_desc(x: "Blob", y: "Blob", g: DwGeom, w: Optional[int] = None, bias: Optional[int] = None, flags: int = 0) -> L.DwConvDesc:
    """fcn_dwconv_desc of the FORWARD problem `g`: x the view of the layer's input (or of its gradient: the data-gradient pass writes
    it), y the view of its output (or of dY), w the tap-major bank."""
    return L.dwconv_desc(x.ptr, w, bias, y.buf.ptr, g.n, g.h, g.w, g.c, x.cstride, g.kh, g.kw, g.ph, g.pw, g.sh, g.sw, g.d,
                         y.cstride, y.coffset, flags)


class DeviceBuffer:
    """Owns one hipMalloc allocation."""

    def __init__(self, nbytes: int, zero: bool = True):
        p = C.c_void_p()
        L.call("fcn_malloc", C.byref(p), nbytes)
        self.ptr = int(p.value)
        self.nbytes = int(nbytes)
        if zero:
            L.call("fcn_memset_async", self.ptr, 0, self.nbytes, None)
            L.call("fcn_device_sync")

    def free(self) -> None:
        if getattr(self, "ptr", 0):
            try:
                L.load().fcn_free(self.ptr)
            finally:
                self.ptr = 0

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class DevView:
    """A slice of a DeviceBuffer (no ownership)."""

    __slots__ = ("ptr", "nbytes")

    def __init__(self, ptr: int, nbytes: int):
        self.ptr, self.nbytes = int(ptr), int(nbytes)


class PinnedArray:
    """A numpy float32 array backed by hipHostMalloc memory (stable address for graph memcpy nodes)."""

    def __init__(self, shape: Tuple[int, ...]):
        n = int(np.prod(shape)) if len(shape) else 1
        p = C.c_void_p()
        L.call("fcn_host_malloc", C.byref(p), max(n, 1) * 4)
        self.ptr = int(p.value)
        buf = (C.c_float * max(n, 1)).from_address(self.ptr)
        self.array = np.frombuffer(buf, dtype=F32, count=n).reshape(shape)
        self.array[...] = 0

    def free(self) -> None:
        if getattr(self, "ptr", 0):
            self.array = None
            try:
                L.load().fcn_host_free(self.ptr)
            finally:
                self.ptr = 0

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class Blob:
    """One named blob: NCHW shape, NHWC device view (buffer, channel offset, channel stride)."""

    def __init__(self, name: str, shape: Tuple[int, ...]):
        self.name = name
        self.shape = tuple(shape)
        self.buf: Optional[DeviceBuffer] = None
        self.coffset = 0
        self.cstride = 0
        self.esize = 4                 # bytes per element on the device: 4 (float32) or 2 (half, Engine(dtype="f16"))
        self.lazy_shift = 0.0          # value added when the blob is read back (Power layer folded into the upload)
        self.upload_shift = 0.0        # value added while the blob is uploaded (device copy = host + upload_shift)
        self.host: Optional[np.ndarray] = None
        self.pinned: Optional[PinnedArray] = None
        self.host_valid = False        # host copy reflects the device contents
        self.is_input = False
        self.rows = False              # an (N,) label blob of a loss / Accuracy over N score rows: N pixels of one channel

    @property
    def nchw(self) -> Optional[Tuple[int, int, int, int]]:
        """The blob as the NHWC machinery sees it (storage.blob_nchw): N x C x H x W, or None for dense floats outside it."""
        return S.blob_nchw(self.shape, self.rows)

    @property
    def channels(self) -> int:
        return self.nchw[1] if self.nchw is not None else 1

    @property
    def pixels(self) -> int:
        g = self.nchw
        return g[0] * g[2] * g[3] if g is not None else 1

    @property
    def ptr(self) -> int:
        """Device address of channel 0 of pixel 0 of this view."""
        return self.buf.ptr + self.esize * self.coffset

    @property
    def contiguous(self) -> bool:
        return self.coffset == 0 and self.cstride == self.channels


class Op:
    """One launch (or fused group of launches) of the plan."""

    def __init__(self, kind: str, name: str, run: Callable[[Optional[int]], None], flops: float = 0.0, bytes_: float = 0.0):
        self.kind = kind
        self.name = name
        self.run = run
        self.flops = flops
        self.bytes = bytes_


Range = Tuple[int, int, int]      # (buffer address, first channel, one past the last channel) of a blob view


@dataclass(eq=False)
class ConvTask:
    """A convolution of the forward plan: a descriptor for the grouped launch of its level."""
    layer: Layer
    desc: L.ConvDesc
    flops: float
    bytes: float
    reads: List[Range]
    writes: List[Range]


@dataclass(eq=False)
class OpTask:
    """Any other layer (or fused run of layers) that launches something: its ops; pool_desc if it is a MAX pooling that can
    ride in a convolution launch; rconv if it is a dilated or rectangular Convolution (its ops are made when its level is emitted:
    those of one level that read one bottom share a launch, _emit_rconvs)."""
    layer: Layer
    ops: List[Op]
    reads: List[Range]
    writes: List[Range]
    pool_desc: Optional[L.PoolDesc] = None
    rconv: Optional[L.RConvDesc] = None      # a dilated or rectangular Convolution (csrc/rconv.hip)
    dwconv: Optional[L.DwConvDesc] = None    # a depthwise Convolution (csrc/dwconv.hip): the descriptor its one op launches


Task = Union[ConvTask, OpTask]


@dataclass(eq=False)
class BnChain:
    """A fused run BatchNorm -> Scale -> ReLU (any part may be missing, BatchNorm or Scale comes first): x the blob it reads, y the
    one it writes, mids the tops in between that the fused launch never writes.  save: mean, invstd and the two backward sums of a
    BatchNorm, 4 x r4(C) floats."""
    x: str
    y: str
    bn: Optional[Layer] = None
    scale: Optional[Layer] = None
    relu: Optional[Layer] = None
    mids: List[str] = field(default_factory=list)
    save: Optional["DeviceBuffer"] = None
    global_stats: bool = False


@dataclass(eq=False)
class ArgChain:
    """An ArgMax and what one launch takes in with it (csrc/argmax.hip): an Interp and / or a Softmax directly in front, each read by
    the next link alone.  x: the blob the launch reads, y: the ArgMax top, mids: the tops in between, which the launch never writes."""
    x: str
    y: str
    argmax: Optional[Layer] = None
    interp: Optional[Layer] = None
    softmax: Optional[Layer] = None
    mids: List[str] = field(default_factory=list)


def ranges_hit(a: Sequence[Range], b: Sequence[Range]) -> bool:
    return any(x[0] == y[0] and x[1] < y[2] and y[1] < x[2] for x in a for y in b)


def task_waits(later: Task, earlier: Task) -> bool:
    """`later` reads what `earlier` writes, or overwrites what it writes or reads."""
    return ranges_hit(later.reads, earlier.writes) or ranges_hit(later.writes, earlier.writes) or ranges_hit(later.writes, earlier.reads)


def task_levels(tasks: Sequence[Task], group_convs: bool = True) -> List[int]:
    """Dependency level of every task (layer order in, so a task waits only for earlier ones): tasks on one level are mutually
    independent.  group_convs False: strict layer order, one level per task."""
    levels: List[int] = []
    for i, ti in enumerate(tasks):
        levels.append(max([levels[j] + 1 for j in range(i) if task_waits(ti, tasks[j])], default=0) if group_convs else i)
    return levels


def task_floats(tasks: Sequence[Task], levels: Sequence[int], i: int) -> bool:
    """Nothing of the next level waits for task i: it may run on that level as well."""
    return not any(levels[j] == levels[i] + 1 and task_waits(tj, tasks[i]) for j, tj in enumerate(tasks) if j != i)


class Engine:
    """Executes a NetSpec on one GPU through libfcnhip.so."""

    def __init__(self, spec: NetSpec, data_shapes: Optional[Dict[str, Tuple[int, ...]]] = None,
                 params: Optional[Dict[str, List[np.ndarray]]] = None, device: int = 0,
                 fuse: bool = True, group_convs: bool = True, autotune: bool = True, dtype: str = "f32",
                 tune_from: Optional["Engine"] = None, tune_max_lds_kb: Optional[int] = None,
                 share_params: Optional["Engine"] = None, score_outputs: bool = False, replica: Optional[int] = None, **state):
        """replica: this engine is replica number `replica` of a frame pipeline and takes a replica stream (default: the next
        number of an enclosing `replica_streams()` context, else a plain stream).
        share_params: Net::ShareTrainedLayersWith - every parameter layer whose name the given engine also has reads that
        engine's flat parameter buffer in place (no copy; a solver step is visible to the next forward of this engine).
        score_outputs: the engine is built for scoring (Solver::Test, `caffe test`): every forward also adds each output blob
        to a device accumulator (score_begin() / forward_score() / score_read()).
        state: what a subclass's _init_state takes besides (a TrainEngine's solver and comm)."""
        self._init_state(spec, data_shapes, dtype=dtype, fuse=fuse, group_convs=group_convs, autotune=autotune, share_params=share_params,
                         score_outputs=score_outputs, **state)
        self.device = device
        L.call("fcn_init", device)
        sp = C.c_void_p()
        self.replica = replica if replica is not None else _take_replica_index()
        if self.replica is None:
            L.call("fcn_stream_create", C.byref(sp))
        else:
            L.call("fcn_stream_create_replica", C.byref(sp), int(self.replica))
        self.stream = int(sp.value)
        yes = C.c_int(0)
        L.call("fcn_stream_is_prioritized", self.stream, C.byref(yes))
        self.stream_prioritized = bool(yes.value)      # False on a replica: the runtime refused, its queue is shared again
        # autotuner: only tile configurations whose workgroup holds at most this much LDS (engines that share the GPU with
        # other streams: small footprints let workgroups of concurrent launches fit on a CU side by side)
        max_lds = int(tune_max_lds_kb if tune_max_lds_kb is not None else os.environ.get("FCN_TUNE_MAX_LDS_KB", "160")) * 1024
        # tune_from: a replica of the same net, whose plan is reused instead of timing again
        self.tuner = T.Tuner(self.stream, T.key_suffix(self.shapes.get(self.inputs[0], ()) if self.inputs else None, self.f16, max_lds),
                             spec.phase == "TEST", max_lds, tune_from._chosen_cfgs if tune_from is not None else None)
        self._plan_buffers()
        self._alloc_params(params)
        self._build_ops()
        self.tuner.release()      # (a TrainEngine tunes its backward plan after this, and releases again)

    def _init_state(self, spec: NetSpec, data_shapes: Optional[Dict[str, Tuple[int, ...]]] = None, *, dtype: str = "f32", fuse: bool = True,
                    group_convs: bool = True, autotune: bool = True, share_params: Optional["Engine"] = None, score_outputs: bool = False) -> None:
        """The host-side state every planner reads, declared once: the argument checks, the inferred shapes, and an empty value for each
        dict, list, set and handle that __init__, the planners and close() use.  No device call, no buffer, no tuner: __init__ makes
        those after it, and a test that plans without a GPU (tests/plan_stub.py) starts from here."""
        if dtype not in ("f32", "f16"):
            raise ValueError("dtype must be 'f32' or 'f16'")
        if share_params is not None and (dtype != "f32" or share_params.f16):
            raise NotImplementedError("share_params: only between float32 engines (a half-float engine packs its weights differently)")
        self._share_from = share_params
        self.shared_layers: set = set()
        self.score_outputs = bool(score_outputs)
        self.score_acc: Dict[str, DeviceBuffer] = {}
        self.graph_score: Optional[int] = None
        if dtype == "f16" and spec.phase != "TEST":
            raise NotImplementedError("the half-float path is inference only (BASELINE configs[4])")
        self.dtype, self.f16 = dtype, dtype == "f16"      # f16: activations / weights stored as halves, f32 accumulation
        self.spec = spec
        self.fuse = fuse
        self.group_convs = group_convs
        self.autotune = autotune
        self.stream = None
        self.lock = threading.RLock()
        self.shapes = spec.infer(data_shapes)
        self.blobs: Dict[str, Blob] = {}
        self.params_host: Dict[str, List[np.ndarray]] = {}
        self.params_dev: Dict[str, List[DevView]] = {}
        self.ops: List[Op] = []
        self.graph_io: Optional[int] = None
        self.graph_core: Optional[int] = None
        self._staging: Dict[str, DeviceBuffer] = {}
        self._keep: List[object] = []
        self._conv_layer_meta: Dict[str, dict] = {}
        self._group_workspaces: List[DeviceBuffer] = []      # workspaces of prepared launch groups (released on close)
        self.aux_dev: Dict[str, DeviceBuffer] = {}      # TRAIN: pooling argmax / LRN scale / BatchNorm x-hat kept for backward
        self._bn_chains: Dict[str, BnChain] = {}        # first layer of a BatchNorm / Scale / ReLU chain -> the chain
        self._bn_ws_bytes = 0                           # the largest fcn_batchnorm_workspace_bytes over the net's layers
        self._bn_ws: Optional[DeviceBuffer] = None
        self._lazy_blob_ops: Dict[str, List[Op]] = {}   # blobs that fused launches do not write -> the launches that do
        self.loss_blobs: Dict[str, float] = {}          # loss top -> loss_weight
        self.device_fed: set = set()             # input blobs a producer writes straight into HBM (device scene renderer): never uploaded
        self.dropout_seed = 0
        self.dropout_index_offset = 0           # data-parallel rank r: r * (elements of the dropout blob)
        self.inputs = spec.data_tops()
        # (a pooling mask that no Upsample consumes is no output: it is not an activation blob; read_blob() still returns it)
        self.outputs = [b for b in spec.output_blobs() if b in self.shapes and b not in spec.mask_blobs]

    @property
    def _chosen_cfgs(self) -> Dict[str, object]:
        """What the autotuner decided: cache key -> tile configuration, or the code of a cut / a move."""
        return self.tuner.chosen

    # ------------------------------------------------------------------ buffers
    def _plan_buffers(self) -> None:
        """One DeviceBuffer per blob that owns its storage, every other blob a channel window of one: storage.plan_blobs decides."""
        plan = S.plan_blobs(self.spec, self.shapes, self.inputs, self.outputs, self.f16, self.fuse, os.environ.get("FCN_F16_IMAGE", "1") != "0")
        self.producers, self.consumers = plan.producers, plan.consumers
        self.alias, self.shift, self.copy_concats, self.copy_slices = plan.alias, plan.shift, plan.copy_concats, plan.copy_slices
        self._half_inputs = plan.half_inputs      # data top -> (Power top, shift)
        self.permutes, self.gathers, self.detections = plan.permutes, plan.gathers, plan.detections      # SSD heads (storage.BlobPlan)
        self.pair_softmax, self.rpn_views = plan.pair_softmax, plan.rpn_views                            # the RPN softmax chain
        # Proposal layer -> the device int32 that holds how many of its post_nms_topn rows the last forward found, and its host copy
        self.roi_counts: Dict[str, DeviceBuffer] = {}
        self._roi_count_host: Dict[str, "PinnedArray"] = {}
        self._roi_caps: Dict[str, int] = {}
        self._counts_valid = False
        bufs = {root: DeviceBuffer(nbytes) for root, nbytes in plan.root_bytes.items()}
        for name, v in plan.views.items():
            b = self.blobs[name] = Blob(name, v.shape)
            b.esize, b.rows, b.is_input = v.esize, v.rows, name in self.inputs
            b.buf, b.coffset, b.cstride = bufs[v.root], v.coffset, v.cstride
            b.upload_shift, b.lazy_shift = v.upload_shift, v.lazy_shift
        self._upload_priors()
        for d in self._half_inputs:                 # the two constant-1 channels, once: every writer of the image touches channels 0..2 only
            b = self.blobs[d]
            ones = np.zeros((b.pixels, b.cstride), np.float16)
            ones[:, 3:5] = 1.0
            L.call("fcn_memcpy_h2d_async", b.buf.ptr, ones.ctypes.data, ones.nbytes, None)
            L.call("fcn_device_sync")

    def _upload_priors(self) -> None:
        """The tops of the PriorBox layers and of their Concat(axis 2) are constants of the plan: computed here by ssd.prior_boxes, uploaded
        once, never touched by forward().  prior_consts keeps the host copies (read_blob returns them)."""
        self.prior_consts: Dict[str, np.ndarray] = {}
        for name, l in self.spec.prior_blobs.items():
            if l.type == "PriorBox":
                _, _, fh, fw = self.shapes[l.bottoms[0]]
                _, _, dh, dw = self.shapes[l.bottoms[1]]
                a = SSD.prior_boxes(SSD.priorbox_params(l), fh, fw, dh, dw)
            else:
                a = np.concatenate([self.prior_consts[b] for b in l.bottoms], axis=2)
            if a.shape != tuple(self.shapes[name]):
                raise RuntimeError("layer %s: %s prior constants for the blob %s" % (l.name, a.shape, self.shapes[name]))
            self.prior_consts[name] = a = np.ascontiguousarray(a, F32)
            b = self.blobs[name]
            if b.coffset or b.cstride != a.size:
                raise NotImplementedError("layer %s: the prior blob %s is a window of another buffer" % (l.name, name))
            L.call("fcn_memcpy_h2d_async", b.buf.ptr, a.ctypes.data, a.nbytes, None)
            L.call("fcn_device_sync")

    def _alloc_params(self, params: Optional[Dict[str, List[np.ndarray]]]) -> None:
        """All learnable blobs live in ONE flat device buffer in the kernels' layout (conv weights OHWI with Cin padded
        to 4): the solver update and the gradient all-reduce are then single launches over one buffer."""
        from .netspec import fill_params
        if params is None:
            params = fill_params(self.spec, seed=0)
        self.param_segs: Dict[Tuple[str, int], S.ParamSeg] = {}      # (layer, blob index) -> its segment, shared layers' included
        src = self._share_from
        if src is not None:
            # shared layers: views INTO the source's flat buffer (the packed bytes of a float32 layer do not depend on the phase:
            # OHWI with Cin padded to 4 / the depthwise deconvolution's filters as they are).  Holding the source's DeviceBuffers
            # keeps the storage alive whichever engine is closed or collected first; this engine never writes or frees it.
            self._shared_keep = [src.param_flat] + list(getattr(src, "_shared_keep", []))
            for l in self.spec.param_layers():
                if l.name not in src.params_dev:
                    continue
                mine, theirs = [tuple(x) for x in self.spec.param_shapes[l.name]], [tuple(x) for x in src.spec.param_shapes[l.name]]
                if mine != theirs:
                    raise ValueError("share_params: layer %s has blobs %s here and %s in the source net" % (l.name, mine, theirs))
                self.shared_layers.add(l.name)
                self.params_host[l.name] = src.params_host[l.name]
                self.params_dev[l.name] = [DevView(v.ptr, v.nbytes) for v in src.params_dev[l.name]]
                self.param_segs.update({(l.name, i): src.param_segs[(l.name, i)] for i in range(len(mine))})
        # the device layout of every blob this engine owns (storage.py): kernels' layout, offsets in 4-byte words
        self.param_layout, self.param_count = S.param_layout(self.spec, self.blobs, self.f16, self.shared_layers)
        for l in self.spec.param_layers():
            if l.name in self.shared_layers:
                continue
            shapes = self.spec.param_shapes[l.name]
            blobs = params.get(l.name)
            if blobs is None:
                raise KeyError("no parameters for layer %s" % l.name)
            host = []
            for arr, shp in zip(blobs, shapes):
                a = np.ascontiguousarray(arr, dtype=F32)
                if a.shape != tuple(shp):
                    if a.size != int(np.prod(shp)):
                        raise ValueError("layer %s: parameter shape %s does not match %s" % (l.name, a.shape, shp))
                    a = a.reshape(shp)
                host.append(a.copy())
            self.params_host[l.name] = host
        self.param_flat = DeviceBuffer(max(self.param_count, 4) * 4, zero=True)
        for seg in self.param_layout:
            self.param_segs[(seg.layer, seg.index)] = seg
            self.params_dev.setdefault(seg.layer, []).append(DevView(self.param_flat.ptr + 4 * seg.offset, seg.nbytes))
        for l in self.spec.param_layers():
            if l.name not in self.shared_layers:
                self._upload_params(l)

    def _folded_shift(self, l: Layer) -> float:
        """The Power shift that convolution l carries in channels 3 and 4 of its filters: its bottom is the Power top of a half image."""
        return next((sh for t, sh in self._half_inputs.values() if t == l.bottoms[0]), 0.0) if l.type == "Convolution" else 0.0

    def _upload_params(self, l: Layer) -> None:
        if l.name in self.shared_layers:
            raise RuntimeError("layer %s reads the parameters of another engine (share_params): set them there" % l.name)
        packed = [S.pack(self.param_segs[(l.name, i)], h, self._folded_shift(l) if i == 0 else 0.0) for i, h in enumerate(self.params_host[l.name])]
        for arr, dev in zip(packed, self.params_dev[l.name]):
            L.call("fcn_memcpy_h2d_async", dev.ptr, arr.ctypes.data, arr.nbytes, None)
        L.call("fcn_device_sync")

    def set_params(self, layer: str, blobs: Sequence[np.ndarray]) -> None:
        """Replace a layer's parameter blobs (Caffe layouts: conv OIHW + bias) and re-upload."""
        lay = next(l for l in self.spec.layers if l.name == layer)
        if layer in self.shared_layers:
            raise RuntimeError("layer %s reads the parameters of another engine (share_params): set them there" % layer)
        shapes = self.spec.param_shapes[layer]
        self.params_host[layer] = [np.ascontiguousarray(b, dtype=F32).reshape(s).copy() for b, s in zip(blobs, shapes)]
        self._upload_params(lay)

    def read_param(self, layer: str, index: int) -> np.ndarray:
        """Caffe-layout host copy (conv: OIHW, bias) of one parameter blob as the device holds it now - for a shared layer, the
        source engine's current weights."""
        with self.lock:
            v = self.params_dev[layer][index]
            raw = np.empty(v.nbytes, np.uint8)
            L.call("fcn_memcpy_d2h_async", raw.ctypes.data, v.ptr, raw.nbytes, self.stream)
            L.call("fcn_stream_sync", self.stream)
        return S.unpack(self.param_segs[(layer, index)], raw)

    # ------------------------------------------------------------------ plan
    def _geom(self, l: Layer, ksp: Optional[Tuple[int, int, int]] = None) -> ConvGeom:
        """Geometry of a Convolution / Deconvolution / Pooling layer from its blobs and its kernel_size / stride / pad (`ksp`
        overrides the three: global pooling)."""
        n, cin, h, w = self.blobs[l.bottoms[0]].shape
        _, cout, oh, ow = self.blobs[l.tops[0]].shape
        k, s, pad = ksp or kernel_stride_pad(l.sub("pooling_param" if l.type == "Pooling" else "convolution_param"))
        return ConvGeom(n, cin, h, w, cout, oh, ow, k, s, pad)

    def _rgeom(self, l: Layer) -> RectGeom:
        """Per-axis geometry of a rectangular Convolution (netspec.is_rectangular) from its blobs and netspec.layer_geometry."""
        n, cin, h, w = self.blobs[l.bottoms[0]].shape
        _, cout, oh, ow = self.blobs[l.tops[0]].shape
        return RectGeom(n, cin, h, w, cout, oh, ow, *layer_geometry(l), layer_dilation(l))

    def _dwgeom(self, l: Layer) -> DwGeom:
        """Per-axis geometry of a depthwise Convolution (NetSpec.is_depthwise) from its blobs and netspec.layer_geometry."""
        n, c, h, w = self.blobs[l.bottoms[0]].shape
        _, _, oh, ow = self.blobs[l.tops[0]].shape
        return DwGeom(n, c, h, w, oh, ow, *layer_geometry(l), layer_dilation(l))

    def _conv_groups(self, l: Layer) -> int:
        """`group` of a Convolution (storage.conv_groups decided, and refused, when the parameters were laid out)."""
        return int(l.sub("convolution_param").get("group", 1)) if l.type == "Convolution" else 1

    def _conv_desc(self, l: Layer, fused_relu: bool, sig_top: Optional[str], group: int = 0) -> L.ConvDesc:
        """The descriptor of convolution l, or of its group `group`: a group is an ordinary problem of Cin/g inputs and Cout/g outputs
        whose x, bank, bias and y_coffset are advanced to the group's channels and rows (storage.conv_groups)."""
        g, ng = self._geom(l), self._conv_groups(l)
        xb, yb = self.blobs[l.bottoms[0]], self.blobs[l.tops[0]]
        eps = 16 // xb.esize
        if xb.coffset % eps or xb.cstride % eps:
            raise NotImplementedError("conv input view of %s is not 16-byte aligned" % l.name)
        flags = 0
        if xb.esize == 2:
            flags |= L.CONV_F16 | (L.CONV_OUT_F32 if yb.esize == 4 else 0)
            # the half image of _half_inputs: channels 3 and 4 are the constant 1 (written once, _plan_buffers), 5..7 stay zero and
            # storage.pack puts the folded shift into the filters' channels 3 and 4 - the first-layer kernel may take them as constants
            if self._folded_shift(l) and _ra(g.cin, 2) == 8 and xb.cstride == 8:
                flags |= L.CONV_IMAGE_ONES
        elif yb.esize != 4:
            flags |= L.CONV_OUT_F16      # first layer of an f16 net: float32 image in, halves out
        if fused_relu:
            flags |= L.CONV_RELU
        if sig_top:
            flags |= L.CONV_SIGMOID2
        pd = self.params_dev[l.name]
        cin_g, cout_g = g.cin // ng, g.cout // ng
        d = conv_desc(xb, yb, g._replace(cin=_ra(cin_g, xb.esize), cout=cout_g), pd[0].ptr, pd[1].ptr if len(pd) > 1 else None, flags)
        if ng > 1:
            if sig_top or self._folded_shift(l) or cout_g % (16 // yb.esize):
                raise NotImplementedError("grouped Convolution %s: a fused Sigmoid, a folded input shift or output groups of %d channels "
                                          "that split a 16-byte segment of the top" % (l.name, cout_g))
            d.x += xb.esize * group * cin_g
            d.w += xb.esize * group * cout_g * g.k * g.k * cin_g
            if d.bias:
                d.bias += 4 * group * cout_g
            d.y_coffset += group * cout_g
        if sig_top:
            sb = self.blobs[sig_top]
            if sb.esize != 4:
                raise NotImplementedError("sigmoid output %s must be float32" % sig_top)
            d.y2, d.y2_cstride, d.y2_coffset = sb.buf.ptr, sb.cstride, sb.coffset
        return d

    def _range(self, name: str) -> Tuple[int, int, int]:
        pool = self.spec.mask_blobs.get(name)
        if pool is not None:      # a pooling mask: the layer's argmax buffer, written by the pooling and read by its Upsample layers
            return (self.aux_dev[pool.name].ptr, 0, max(self.shapes[name][1], 1))
        b = self.blobs[name]
        return (b.buf.ptr, b.coffset, b.coffset + max(b.channels, 1))

    def _relu_after(self, li: int, l: Layer, skip: set) -> bool:
        """True when the first layer that touches l's top is an in-place ReLU without a negative slope: it rides in l's epilogue
        (Convolution, InnerProduct) and joins `skip`."""
        top = l.tops[0]
        if not self.fuse:
            return False
        for nxt in self.spec.layers[li + 1:]:
            if top in nxt.bottoms or top in nxt.tops:
                if nxt.type == "ReLU" and nxt.bottoms == [top] and nxt.tops == [top] and \
                        float(nxt.sub("relu_param").get("negative_slope", 0.0)) == 0.0:
                    skip.add(nxt.name)
                    return True
                break
        return False

    def _fused_after(self, li: int, l: Layer, skip: set) -> Tuple[bool, Optional[str]]:
        """(an in-place ReLU directly after convolution l rides in its epilogue, the top of a Sigmoid that does) - the layers so
        absorbed join `skip`."""
        top = l.tops[0]
        if not self.fuse:
            return False, None
        if self._relu_after(li, l, skip):
            return True, None
        cons = self.consumers.get(top, [])
        if len(cons) == 1 and cons[0].type == "Sigmoid" and cons[0].tops[0] != top and len(self.producers.get(top, [])) == 1:
            skip.add(cons[0].name)
            return False, cons[0].tops[0]
        return False, None

    def _bn_chain_after(self, li: int, l: Layer, skip: set) -> "BnChain":
        """The chain BatchNorm -> Scale -> ReLU (negative_slope 0) that starts at layer l (a BatchNorm or a Scale): a link joins while it
        is the first layer after its predecessor that touches the predecessor's top, and - when it writes a top of its own - the only
        consumer of that blob, which is no output of the net (the fused launch never writes it).  In place (the ResNet prototxts) and
        with separate tops (the reference's commented-out pairs).  Absorbed layers join `skip`, like _relu_after's."""
        ch = BnChain(l.bottoms[0], l.tops[0])
        setattr(ch, "bn" if l.type == "BatchNorm" else "scale", l)
        last = l
        want = ["Scale", "ReLU"] if l.type == "BatchNorm" else ["ReLU"]
        while self.fuse and want:
            top = last.tops[0]
            nxt = next((q for q in self.spec.layers[self.spec.layers.index(last) + 1:] if top in q.bottoms or top in q.tops), None)
            if nxt is None or nxt.type not in want or nxt.bottoms != [top] or len(nxt.tops) != 1:
                break
            if nxt.type == "ReLU" and float(nxt.sub("relu_param").get("negative_slope", 0.0)) != 0.0:
                break
            if nxt.tops[0] != top and ([q.name for q in self.consumers.get(top, [])] != [nxt.name] or top in self.outputs
                                       or len(self.producers.get(top, [])) != 1 or top in self.alias or nxt.tops[0] in self.alias):
                break
            if nxt.tops[0] != top:
                ch.mids.append(top)
            setattr(ch, "scale" if nxt.type == "Scale" else "relu", nxt)
            skip.add(nxt.name)
            ch.y = nxt.tops[0]
            last = nxt
            want = want[want.index(nxt.type) + 1:]
        return ch

    def _bn_apply_op(self, name: str, xb: Blob, yb: Blob, ch: "BnChain", scale: bool, relu: bool, xhat: Optional[DeviceBuffer]) -> Op:
        """One launch y = relu?(gamma * (x - mean) * invstd + beta) of the chain ch (csrc/batchnorm.hip), any of its parts left out."""
        lib = L.load()
        pix, c = xb.pixels, xb.channels
        bn = self.params_dev[ch.bn.name] if ch.bn is not None else None
        sc = self.params_dev[ch.scale.name] if scale and ch.scale is not None else None
        eps = float(ch.bn.sub("batch_norm_param").get("eps", 1e-5)) if ch.bn is not None else 0.0
        save = ch.save.ptr if ch.save is not None and not ch.global_stats else None
        blobs = [v.ptr for v in bn] if bn is not None and save is None else [None, None, None]
        gamma, beta = (sc[0].ptr if sc else None), (sc[1].ptr if sc and len(sc) > 1 else None)
        if xb.esize == 2:
            return Op("bn_apply", name, lambda st: L.check(lib.fcn_batchnorm_apply_f16(
                xb.buf.ptr, yb.buf.ptr, pix, c, xb.cstride, xb.coffset, yb.cstride, yb.coffset, *blobs, eps, gamma, beta, int(relu), st)),
                4.0 * pix * c, 4.0 * pix * c)
        hp = xhat.ptr if xhat is not None else None
        return Op("bn_apply", name, lambda st: L.check(lib.fcn_batchnorm_apply_f32(
            xb.buf.ptr, yb.buf.ptr, hp, pix, c, xb.cstride, xb.coffset, yb.cstride, yb.coffset, _r4(c), save, *blobs, eps, gamma, beta,
            int(relu), st)), 4.0 * pix * c, (8.0 + (4.0 if hp else 0.0)) * pix * c)

    def _fwd_batchnorm(self, ch: "BnChain") -> List[Op]:
        """Forward of a BatchNorm / Scale / ReLU chain: in TRAIN with batch statistics the statistics launch (which also moves the three
        blobs: part of every TRAIN forward, inside the step graph) and ONE apply launch; otherwise the apply launch alone, which takes
        mean and invstd from the blobs in its prologue - a TEST engine that shares a training net's blobs sees the current averages.
        TRAIN keeps x-hat (for Scale alone in place: its input) in aux_dev, as pooling keeps its argmax."""
        lib, B = L.load(), self.blobs
        first = ch.bn or ch.scale
        xb, yb = B[ch.x], B[ch.y]
        if xb.nchw is None or xb.shape != yb.shape:
            raise NotImplementedError("%s %s on a blob that is neither 4-d nor 2-d" % (first.type, first.name))
        if xb.esize != yb.esize or any(B[m].esize != xb.esize for m in ch.mids):
            raise NotImplementedError("f16 engine: %s %s between half and float32 blobs" % (first.type, first.name))
        eps_g = 16 // xb.esize
        if xb.coffset % eps_g or yb.coffset % eps_g or xb.cstride % eps_g or yb.cstride % eps_g:
            raise NotImplementedError("%s %s: a channel window that is not 16-byte aligned" % (first.type, first.name))
        pix, c = xb.pixels, xb.channels
        ch.global_stats = ch.bn is not None and bn_global_stats(ch.bn, self.spec.phase)
        if xb.esize == 2 and ch.bn is not None and not ch.global_stats:
            raise NotImplementedError("f16 engine: BatchNorm %s with batch statistics (half floats are inference only)" % ch.bn.name)
        train = self.spec.phase == "TRAIN"
        ops: List[Op] = []
        name = "+".join(q.name for q in (ch.bn, ch.scale, ch.relu) if q is not None)
        if ch.bn is not None and (train or not ch.global_stats):
            # mean, invstd, then (backward, BatchNorm without a learning Scale) sum dy', sum dy' x-hat: four runs of C floats
            ch.save = DeviceBuffer(4 * _r4(c) * 4, zero=True)
            self._keep.append(ch.save)
        if train or (ch.bn is not None and not ch.global_stats):      # one workspace for every reducing launch of the net, forward and backward
            self._bn_ws_bytes = max(self._bn_ws_bytes, int(lib.fcn_batchnorm_workspace_bytes(pix, c)))
        if ch.bn is not None and not ch.global_stats:
            f = float(ch.bn.sub("batch_norm_param").get("moving_average_fraction", 0.999))
            eps = float(ch.bn.sub("batch_norm_param").get("eps", 1e-5))
            bm, bv, bf = (v.ptr for v in self.params_dev[ch.bn.name])
            ops.append(Op("bn_stats", ch.bn.name, lambda st: L.check(lib.fcn_batchnorm_stats_f32(
                xb.buf.ptr, pix, c, xb.cstride, xb.coffset, bm, bv, bf, f, eps, ch.save.ptr, self._bn_ws.ptr, st)), 6.0 * pix * c, 8.0 * pix * c))
        xhat = None
        need = getattr(self, "need_grad", None)
        if train and (need is None or ch.y in need) and (ch.bn is not None or ch.x == ch.y):
            xhat = self.aux_dev[first.name] = DeviceBuffer(pix * _r4(c) * 4, zero=True)
        ops.append(self._bn_apply_op(name, xb, yb, ch, True, ch.relu is not None, xhat))
        # the tops in the middle of a chain with separate tops own a buffer that the fused launch leaves alone: read_blob() fills it on demand
        for m in ch.mids:
            self._lazy_blob_ops[m] = [self._bn_apply_op(m, xb, B[m], ch, ch.scale is not None and m in ch.scale.tops, False, None)]
        self._bn_chains[first.name] = ch
        return ops

    @staticmethod
    def _gate_residual(sc: Layer, elt: Layer) -> str:
        """The bottom of the Eltwise `elt` that is not the top of the gated Scale `sc`."""
        return elt.bottoms[1] if elt.bottoms[0] == sc.tops[0] else elt.bottoms[0]

    def _gate_fusion(self, li: int, l: Layer) -> Optional[Layer]:
        """The Eltwise that takes the gated Scale l into its launch, y = relu?(x * g + r), or None.  TEST-phase engines with `fuse` only.
        The Scale top is read by exactly one layer, an Eltwise SUM of two different bottoms with coefficients 1; it has one producer, is
        no output of the net and no view of another blob (the fused launch never writes it: read_blob() fills it on demand); no layer
        behind the Scale writes x or the gate; and x, the residual and the Eltwise top are windows the kernel takes.  The fused task stands
        at the Eltwise's place in the order (_collect_tasks), where the residual has been written."""
        top, B = l.tops[0], self.blobs
        if not self.fuse or self.spec.phase != "TEST":
            return None
        cons = self.consumers.get(top, [])
        if len(cons) != 1 or top in self.outputs or len(self.producers.get(top, [])) != 1 or top in self.alias or top in l.bottoms:
            return None
        elt = cons[0]
        p = elt.sub("eltwise_param")
        if elt.type != "Eltwise" or str(p.get("operation", "SUM")) != "SUM" or len(elt.bottoms) != 2 or elt.bottoms.count(top) != 1 \
                or any(float(c) != 1.0 for c in p.getall("coeff")) or len(elt.tops) != 1:
            return None
        # nothing behind the Scale may write x or the gate - the Eltwise in place over x included: the fused launch reads them at the
        # Eltwise's place in the order, and read_blob() computes the Scale top from them after the forward pass
        if any(b in q.tops for q in self.spec.layers[li + 1:] for b in l.bottoms):
            return None
        xb, rb, yb = B[l.bottoms[0]], B[self._gate_residual(l, elt)], B[elt.tops[0]]
        grp = 16 // xb.esize
        if any(v.esize != xb.esize or v.nchw is None or v.coffset % grp or v.cstride % grp for v in (xb, rb, yb)):
            return None
        self._gate_fused[elt.name] = l
        return elt

    def _scale_gate_op(self, l: Layer, elt: Optional[Layer], relu: Optional[str]) -> Op:
        """One launch of csrc/gate.hip: y = x * gate[n, c] for the gated Scale l alone (its top), or - with the Eltwise `elt` that
        _gate_fusion found - y = relu?(x * gate[n, c] + r) into the Eltwise top, `relu` the ReLU layer in place behind it.  x, r and y are
        floats or halves alike; the gate is float32 in both engines (the top of a Sigmoid: storage.plan_blobs keeps it so)."""
        lib, B = L.load(), self.blobs
        xb, gb = B[l.bottoms[0]], B[l.bottoms[1]]
        yb = B[elt.tops[0] if elt is not None else l.tops[0]]
        rb = B[self._gate_residual(l, elt)] if elt is not None else None
        n, ppi, c = scale_gate_form(l, [self.shapes[b] for b in l.bottoms], self.spec.phase)
        if self.f16 and l.bottoms[1] in self.inputs:
            raise NotImplementedError("f16 engine: Scale %s takes its multiplier %s from an input of the net" % (l.name, l.bottoms[1]))
        if gb.esize != 4:
            raise NotImplementedError("f16 engine: Scale %s: the multiplier %s is stored as halves (the kernel reads a float32 gate: the top of "
                                      "a Sigmoid is one)" % (l.name, l.bottoms[1]))
        if gb.nchw is None or gb.nchw[0] != n or gb.nchw[1] != c:
            raise NotImplementedError("Scale %s: the multiplier %s is no (N, C) blob on the device" % (l.name, l.bottoms[1]))
        grp = 16 // xb.esize
        for v in (xb, yb) + ((rb,) if rb is not None else ()):
            if v.esize != xb.esize or v.nchw is None or v.coffset % grp or v.cstride % grp:
                raise NotImplementedError("Scale %s: %s is stored in another element type than %s, or is a channel window that is not 16-byte "
                                          "aligned" % (l.name, v.name, xb.name))
        fn = lib.fcn_scale_gate_fwd_f16 if xb.esize == 2 else lib.fcn_scale_gate_fwd_f32
        rp, rcs, rco = (rb.buf.ptr, rb.cstride, rb.coffset) if rb is not None else (None, 0, 0)
        name = l.name if elt is None else "+".join([l.name, elt.name] + ([relu] if relu else []))
        return Op("scale_gate", name, lambda st: L.check(fn(
            xb.buf.ptr, gb.ptr, rp, yb.buf.ptr, n, ppi, c, xb.cstride, xb.coffset, gb.cstride, rcs, rco, yb.cstride, yb.coffset, int(bool(relu)), st)),
            (2.0 if rb is not None else 1.0) * n * ppi * c, float(xb.esize) * (3.0 if rb is not None else 2.0) * n * ppi * c)

    def _argmax_chain_at(self, l: Layer, skip: set) -> Optional["ArgChain"]:
        """The chain [Interp ->] [Softmax ->] ArgMax that starts at layer l, or None when l (an Interp or a Softmax) starts none.  A link
        joins where the blob in front of it has it as its only reader, has one producer, is no output of the net and no view of another
        blob: the fused launch never writes it.  An Interp joins only in front of top_k 1 (the fused pass keeps one pair per pixel).
        Without `fuse` an ArgMax stands alone.  Absorbed layers join `skip`, like _relu_after's."""
        ch, cur = ArgChain(l.bottoms[0], ""), l
        while cur.type != "ArgMax":
            if not self.fuse or len(cur.bottoms) != 1 or len(cur.tops) != 1 or cur.tops[0] == cur.bottoms[0]:
                return None
            if cur.type == "Interp" and ch.interp is None and ch.softmax is None:
                ch.interp = cur
            elif cur.type == "Softmax" and ch.softmax is None and int(cur.sub("softmax_param").get("axis", 1)) == 1 \
                    and len(self.shapes[cur.bottoms[0]]) in (2, 4):
                ch.softmax = cur
            else:
                return None
            top = cur.tops[0]
            cons = self.consumers.get(top, [])
            if len(cons) != 1 or top in self.outputs or len(self.producers.get(top, [])) != 1 or top in self.alias:
                return None
            ch.mids.append(top)
            cur = cons[0]
        ch.argmax, ch.y = cur, cur.tops[0]
        if ch.interp is not None and argmax_form(cur, self.shapes[cur.bottoms[0]])[0] != 1:
            return None
        skip.update(q.name for q in (ch.softmax, ch.argmax) if q is not None and q is not l)
        return ch

    def _fwd_argmax(self, ch: "ArgChain") -> List[Op]:
        """ArgMax as ONE launch, alone or with the Interp and / or the Softmax in front of it.  The top is float32 in both engines; the
        launch reads floats or halves.  The tops in the middle of a chain own a buffer that the launch leaves alone: read_blob() fills
        it on demand with the layers' own launches."""
        lib, B, l = L.load(), self.blobs, ch.argmax
        xb, yb = B[ch.x], B[ch.y]
        top_k, out_max_val, legacy = argmax_form(l, self.shapes[l.bottoms[0]])
        flags = (L.ARGMAX_SOFTMAX if ch.softmax is not None else 0) | ((L.ARGMAX_PAIRS if legacy else L.ARGMAX_VALUES) if out_max_val else 0)
        if yb.esize != 4 or xb.nchw is None:
            raise NotImplementedError("ArgMax %s: the top %s must be float32 and the bottom a 4-d or 2-d blob" % (l.name, ch.y))
        half = xb.esize == 2
        if half and (xb.coffset % 8 or xb.cstride % 8 or yb.coffset % 4 or yb.cstride % 4):
            raise NotImplementedError("f16 engine: ArgMax %s on a channel window that is not 16-byte aligned" % l.name)
        name = "+".join(q.name for q in (ch.interp, ch.softmax, ch.argmax) if q is not None)
        n, c, h, w = xb.nchw
        if ch.interp is not None:
            oh, ow, pad_beg, pad_end = interp_size(ch.interp, h, w)
            fn = lib.fcn_interp_argmax_fwd_f16 if half else lib.fcn_interp_argmax_fwd_f32
            run = lambda st: L.check(fn(xb.buf.ptr, yb.buf.ptr, n, h, w, c, xb.cstride, xb.coffset, pad_beg, pad_end, oh, ow,
                                        yb.cstride, yb.coffset, flags, st))
            byts = float(xb.esize) * n * (h + pad_beg + pad_end) * (w + pad_beg + pad_end) * c
        else:
            fn = lib.fcn_argmax_fwd_f16 if half else lib.fcn_argmax_fwd_f32
            run = lambda st: L.check(fn(xb.buf.ptr, yb.buf.ptr, xb.pixels, c, xb.cstride, xb.coffset, top_k, yb.cstride, yb.coffset, flags, st))
            byts = float(xb.esize) * xb.pixels * c
        lazy: List[Op] = []
        for q, m in zip([q for q in (ch.interp, ch.softmax) if q is not None], ch.mids):
            lazy = lazy + self._emit_simple(q)
            self._lazy_blob_ops[m] = lazy
        return [Op("argmax", name, run, 0.0, byts + 4.0 * yb.pixels * yb.channels)]

    def _collect_tasks(self) -> List[Task]:
        """Layer list -> tasks with read/write sets: one per convolution (a descriptor for the grouped launches) and one per
        other layer that launches anything (its ops)."""
        spec = self.spec
        skip: set = set()
        tasks: List[Task] = []
        self._conv_flags: Dict[str, int] = {}      # Convolution layer of the tiled family -> the CONV_* flags of its descriptor(s)
        self._gate_fused: Dict[str, Layer] = {}    # Eltwise layer -> the gated Scale whose launch it joins (_gate_fusion)
        for li, l in enumerate(spec.layers):
            if l.name in skip:
                continue
            t = l.type
            if t in ("Data", "Python", "Input", "DummyData", "MemoryData", "ImageData", "HDF5Data"):
                continue
            if spec.is_depthwise(l):
                tasks.append(self._dwconv_task(li, l, skip))
                continue
            if t == "Convolution" and (is_rectangular(l) or layer_dilation(l) > 1):
                tasks.append(self._rconv_task(li, l, skip))
                continue
            if t == "Convolution":
                top = l.tops[0]
                fused_relu, sig_top = self._fused_after(li, l, skip)
                g, ng = self._geom(l), self._conv_groups(l)
                # a grouped layer is `group` ordinary problems of one level: each reads and writes its own channels, and together they
                # carry 1/group of the dense layer's FLOPs and weight bytes
                cin_g, cout_g = g.cin // ng, g.cout // ng
                (xp, xlo, _), (yp, ylo, _) = self._range(l.bottoms[0]), self._range(top)
                for i in range(ng):
                    tasks.append(ConvTask(l, self._conv_desc(l, fused_relu, sig_top, i), g.flops / (ng * ng),
                                          4.0 * (g.n * cin_g * g.h * g.w + g.n * cout_g * g.oh * g.ow + cout_g * cin_g * g.k * g.k + cout_g),
                                          reads=[(xp, xlo + i * cin_g, xlo + (i + 1) * cin_g)],
                                          writes=[(yp, ylo + i * cout_g, ylo + (i + 1) * cout_g)] + ([self._range(sig_top)] if sig_top else [])))
                self._conv_layer_meta[l.name] = dict(relu=fused_relu, sigmoid_top=sig_top)
                self._conv_flags[l.name] = int(tasks[-1].desc.flags)
                continue
            if t == "InnerProduct":
                relu = self._relu_after(li, l, skip)
                self._conv_layer_meta[l.name] = dict(relu=relu, sigmoid_top=None)
                tasks.append(OpTask(l, self._fwd_inner_product(l, relu), reads=[self._range(l.bottoms[0])], writes=[self._range(l.tops[0])]))
                continue
            if is_scale_gate(l):      # the multiplier is a blob of the net: csrc/gate.hip, alone or (TEST) with the residual add behind it
                if self._gate_fusion(li, l) is None:
                    tasks.append(OpTask(l, [self._scale_gate_op(l, None, None)], reads=[self._range(b) for b in l.bottoms], writes=[self._range(l.tops[0])]))
                continue
            if t == "Eltwise" and l.name in self._gate_fused:      # (at the Eltwise's place in the order: its residual is written by now)
                sc, before = self._gate_fused[l.name], set(skip)
                relu = next(iter(skip - before)) if self._relu_after(li, l, skip) else None
                self._lazy_blob_ops[sc.tops[0]] = [self._scale_gate_op(sc, None, None)]
                tasks.append(OpTask(l, [self._scale_gate_op(sc, l, relu)], reads=[self._range(b) for b in sc.bottoms + [self._gate_residual(sc, l)]],
                                    writes=[self._range(l.tops[0])]))
                continue
            if t in ("BatchNorm", "Scale"):
                ch = self._bn_chain_after(li, l, skip)
                tasks.append(OpTask(l, self._fwd_batchnorm(ch), reads=[self._range(ch.x)], writes=[self._range(ch.y)]))
                continue
            if t in RG.REGION_TYPES or l.name in self.pair_softmax or (t == "Reshape" and (l.tops[0] in self.rpn_views or l.bottoms[0] in self.rpn_views)):
                tasks.extend(self._region_tasks(l))
                continue
            if t in SSD.HEAD_TYPES or l.name in self.gathers or (l.tops and l.tops[0] in spec.prior_blobs) or \
                    (t == "Softmax" and len(self.shapes[l.bottoms[0]]) == 3 and int(l.sub("softmax_param").get("axis", 1)) in (2, -1)):
                tasks.extend(self._ssd_tasks(l))
                continue
            if t == "Concat" and l.name not in self.copy_concats:
                continue      # producers already wrote their slices
            if t == "Slice" and l.name not in self.copy_slices:
                continue      # tops are views of the bottom
            if t == "Dropout" and spec.phase == "TEST" and (l.tops[0] == l.bottoms[0] or l.tops[0] in self.alias):
                continue
            if t == "Power" and l.tops[0] in self.shift:
                continue      # folded into the consumer convolutions' loaders
            if t in ("Interp", "Softmax", "ArgMax"):
                ch = self._argmax_chain_at(l, skip)
                if ch is not None:
                    tasks.append(OpTask(ch.argmax, self._fwd_argmax(ch), reads=[self._range(ch.x)], writes=[self._range(ch.y)]))
                    continue
            ops = self._emit_simple(l)
            read = l.bottoms[:1] if t == "Crop" else l.bottoms      # a Crop's second bottom is a shape, not data
            tasks.append(OpTask(l, ops, reads=[self._range(b) for b in read], writes=[self._range(tp) for tp in l.tops],
                                pool_desc=self._fusable_pool_desc(l)))
        return tasks

    def _build_ops(self) -> None:
        """Layer list -> tasks with read/write sets -> dependency levels -> launches.

        Tasks on one level are mutually independent; all convolutions of a level share ONE grouped launch
        (an inception module becomes {1x1, 3x3_reduce, 5x5_reduce} then {3x3, 5x5, pool_proj})."""
        tasks = self._collect_tasks()
        if self._bn_ws_bytes:
            self._bn_ws = DeviceBuffer(self._bn_ws_bytes, zero=False)
        if self.fuse and self.spec.phase == "TEST" and os.environ.get("FCN_FUSE_POOL_LRN", "1") != "0":
            tasks = self._fuse_pool_lrn(tasks)
        levels = task_levels(tasks, self.group_convs)
        if self.autotune and self.group_convs and self.fuse and not self.f16 and self.spec.phase == "TEST" and os.environ.get("FCN_LEVEL_MOVE", "1") != "0":
            self.tuner.move_floaters(tasks, levels)
        tail = self._plan_tail(tasks, levels)
        order = sorted(range(len(tasks)), key=lambda i: (levels[i], 1 if isinstance(tasks[i], ConvTask) else 0, i))
        pending: List[ConvTask] = []
        pending_pools: List[OpTask] = []
        pending_rconvs: List[OpTask] = []
        cur = None
        for i in order:
            if levels[i] != cur:
                self._emit_rconvs(pending_rconvs)
                self._emit_convs(pending, pending_pools, tail)
                pending, pending_rconvs, cur = [], [], levels[i]
            if tail is not None and any(tasks[i] is ht for ht in tail["heads"]):
                continue      # evaluated by the launches that produce its input
            if isinstance(tasks[i], ConvTask):
                pending.append(tasks[i])
            elif tasks[i].pool_desc is not None and self.fuse and self.group_convs:
                pending_pools.append(tasks[i])
            elif tasks[i].rconv is not None:
                pending_rconvs.append(tasks[i])
            else:
                self.ops.extend(tasks[i].ops)
        self._emit_rconvs(pending_rconvs)
        self._emit_convs(pending, pending_pools, tail)
        self.levels = max(levels) + 1 if levels else 0
        if self.score_outputs:
            self._emit_score_ops()

    # ------------------------------------------------------------------ SSD detection head (csrc/ssd.hip)
    def _ssd_tasks(self, l: Layer) -> List[OpTask]:
        """The launches of one layer of an SSD head.  Permute, Reshape, the Flatten layers that are views, PriorBox and the priors' Concat emit
        nothing: views and constants of the plan (storage.plan_blobs).  A Concat of Permute + Flatten heads (or such a Flatten on its own) is
        one fcn_ssd_gather_f32 launch per 16 heads; Normalize, the row Softmax and DetectionOutput are one op each."""
        lib, B, t = L.load(), self.blobs, l.type
        need = getattr(self, "need_grad", None)
        if need is not None and any(b in need for b in l.bottoms + l.tops):
            raise NotImplementedError("layer %s: %s below a layer that learns in a TRAIN-phase net (the SSD head has no backward pass: "
                                      "deploy nets only)" % (l.name, t))
        if l.name in self.gathers:
            top, cols = self.gathers[l.name]
            db = B[top]
            n, width = db.shape[0], db.shape[1]
            out: List[OpTask] = []
            for g0 in range(0, len(cols), L.SSD_MAX_HEADS):
                part = cols[g0:g0 + L.SSD_MAX_HEADS]
                arr = (L.SsdHead * len(part))()
                byts = 0.0
                for h, (_flat, src, col) in zip(arr, part):
                    sb = B[src]
                    if sb.esize != 4 or sb.nchw is None or sb.shape[0] != n:
                        raise NotImplementedError("layer %s: the head %s is no float32 4-d blob of %d images" % (l.name, src, n))
                    h.src, h.pixels, h.C, h.cstride, h.coffset, h.dst_col = sb.buf.ptr, sb.shape[2] * sb.shape[3], sb.shape[1], sb.cstride, sb.coffset, col
                    byts += 8.0 * n * h.pixels * h.C
                self._keep.append(arr)
                label = l.name + ":" + "+".join(src for _f, src, _c in part)
                run = lambda st, arr=arr, k=len(part): L.check(lib.fcn_ssd_gather_f32(arr, k, n, db.buf.ptr + 4 * db.coffset, db.cstride, width, st))
                out.append(OpTask(l, [Op("ssd_gather", label, run, 0.0, byts)], reads=[self._range(src) for _f, src, _c in part],
                                  writes=[(db.buf.ptr, db.coffset + part[0][2], db.coffset + part[-1][2] + B[part[-1][0]].channels)]))
            return out
        if t in ("Permute", "Reshape", "Flatten", "PriorBox") or (t == "Concat" and l.tops[0] in self.spec.prior_blobs):
            return []
        if t == "Normalize":
            xb, yb = B[l.bottoms[0]], B[l.tops[0]]
            npar = l.sub("norm_param")
            shared, eps = int(bool(npar.get("channel_shared", True))), float(npar.get("eps", 1e-10))
            scale = self.params_dev[l.name][0]
            if yb.cstride < yb.coffset + _r4(yb.channels):
                raise NotImplementedError("layer %s: the top %s is a channel window that ends inside a 16-byte group" % (l.name, l.tops[0]))
            pix, c = xb.pixels, xb.channels
            run = lambda st: L.check(lib.fcn_normalize_fwd_f32(xb.buf.ptr, yb.buf.ptr, scale.ptr, pix, c, xb.cstride, xb.coffset, yb.cstride,
                                                               yb.coffset, shared, eps, st))
            return [OpTask(l, [Op("normalize", l.name, run, 4.0 * pix * c, 8.0 * pix * c)], reads=[self._range(l.bottoms[0])],
                           writes=[self._range(l.tops[0])])]
        if t == "Softmax":
            # over the last axis of an (N, P, C) blob: P rows of C contiguous floats per image - fcn_softmax_fwd_f32 with pixels = P and both
            # strides C (its lanes load and store single floats: C = 21 needs no alignment), one launch per image (the images' rows start
            # a row stride apart, which is no multiple of C)
            xb, yb = B[l.bottoms[0]], B[l.tops[0]]
            if len(xb.shape) != 3 or not xb.rows or xb.shape != yb.shape:
                raise NotImplementedError("Softmax over an axis other than channels (layer %s)" % l.name)
            n, pr, c = xb.shape
            def run(st):
                for i in range(n):
                    L.check(lib.fcn_softmax_fwd_f32(xb.ptr + 4 * i * xb.cstride, yb.ptr + 4 * i * yb.cstride, pr, c, c, c, st))
            return [OpTask(l, [Op("softmax", l.name, run, 0.0, 8.0 * n * pr * c)], reads=[self._range(l.bottoms[0])], writes=[self._range(l.tops[0])])]
        if t == "DetectionOutput":
            dp = SSD.detection_params(l)
            (_, _, cap, _), priors = SSD.detection_shapes(l, [self.shapes[b] for b in l.bottoms])
            lb, cb, pb, ob = (B[b] for b in l.bottoms + l.tops[:1])
            if pb.coffset or pb.cstride != 8 * priors or any(x.esize != 4 for x in (lb, cb, pb)):
                raise NotImplementedError("layer %s: the priors %s are a window of another buffer" % (l.name, l.bottoms[2]))
            kmax = min(dp.top_k, priors) if dp.top_k > -1 else priors
            if kmax > L.DETOUT_MAX_TOPK:
                raise NotImplementedError("layer %s: DetectionOutput with %d candidates per class (top_k %d over %d priors): the NMS kernel "
                                          "holds at most %d" % (l.name, kmax, dp.top_k, priors, L.DETOUT_MAX_TOPK))
            par = L.DetOutParams()
            par.N, par.P, par.num_classes, par.background = lb.shape[0], priors, dp.num_classes, dp.background
            par.code_type, par.variance_encoded, par.top_k, par.keep_top_k = dp.code_type, int(dp.variance_encoded), dp.top_k, dp.keep_top_k
            par.conf_threshold, par.nms_threshold = dp.confidence_threshold, dp.nms_threshold
            par.loc_rstride, par.conf_rstride, par.capacity = lb.cstride, cb.cstride, cap
            nbytes = int(lib.fcn_detection_output_workspace_bytes(C.byref(par)))
            if nbytes <= 0:
                L.check(lib.fcn_detection_output_f32(None, None, None, C.byref(par), None, None, None, 0, None))      # (raises with the library's text)
                raise RuntimeError("layer %s: DetectionOutput has no plan" % l.name)
            ws = DeviceBuffer(nbytes, zero=True)
            self._keep.extend([ws, par])
            n, nc = par.N, dp.num_classes
            run = lambda st: L.check(lib.fcn_detection_output_f32(lb.ptr, cb.ptr, pb.ptr, C.byref(par), ob.buf.ptr, ob.buf.ptr + 4 * 7 * cap,
                                                                  ws.ptr, nbytes, st))
            return [OpTask(l, [Op("detection_output", l.name, run, 30.0 * n * priors + 20.0 * n * nc * kmax * kmax / 2,
                                  4.0 * n * priors * (4 + nc + 4) + 28.0 * cap)],
                           reads=[self._range(b) for b in l.bottoms], writes=[self._range(l.tops[0])])]
        raise NotImplementedError("layer type %r (layer %s) has no forward kernel yet" % (t, l.name))

    def blob_shape(self, name: str) -> Tuple[int, ...]:
        """A blob's shape as pycaffe reports it: the inferred one - for the top of a DetectionOutput after a forward, (1, 1, K, 7) with the
        K rows that forward found (the inferred shape is the capacity), and for a blob on the ROI axis of a Proposal after a forward, the
        rows that Proposal found in front of the other extents."""
        if name in self.detections and self.blobs[name].host is not None and getattr(self, "_ran", False):
            return self._compose_detections(name).shape
        if name in self.spec.roi_blobs and getattr(self, "_ran", False):
            return (self._roi_count(self.spec.roi_blobs[name].name),) + tuple(self.shapes[name][1:])
        return tuple(self.shapes[name])

    # ------------------------------------------------------------------ region stage (csrc/region.hip)
    def _region_tasks(self, l: Layer) -> List[OpTask]:
        """The launches of one layer of a region stage.  The two Reshape layers of the RPN softmax chain emit nothing: its Softmax layer is
        ONE fcn_pair_softmax_f32 launch from the first Reshape's bottom into the second one's top.  Proposal, ROIPooling and PSROIPooling
        are one op each; Proposal's op is five launches that never wait for the host."""
        lib, B, t = L.load(), self.blobs, l.type
        need = getattr(self, "need_grad", None)
        if need is not None and any(b in need for b in l.bottoms + l.tops):
            raise NotImplementedError("layer %s: %s below a layer that learns in a TRAIN-phase net (the region stage has no backward pass: "
                                      "AnchorTarget, ProposalTarget and the poolings' gradients are not built; deploy nets only)" % (l.name, t))
        if t == "Reshape":
            return []
        if t == "Softmax":
            src, dst, a = self.pair_softmax[l.name]
            xb, yb = B[src], B[dst]
            if xb.esize != 4 or yb.esize != 4 or yb.cstride < yb.coffset + _r4(2 * a):
                raise NotImplementedError("layer %s: the top %s is a channel window that ends inside a 16-byte group" % (l.name, dst))
            pix = xb.pixels
            run = lambda st: L.check(lib.fcn_pair_softmax_f32(xb.buf.ptr, yb.buf.ptr, pix, a, xb.cstride, xb.coffset, yb.cstride, yb.coffset, st))
            return [OpTask(l, [Op("pair_softmax", l.name, run, 0.0, 16.0 * pix * a)], reads=[self._range(src)], writes=[self._range(dst)])]
        if t == "Proposal":
            pp = RG.proposal_params(l)
            RG.proposal_shapes(l, [self.shapes[b] for b in l.bottoms])
            sb, db, ib = (B[b] for b in l.bottoms)
            rb = B[l.tops[0]]
            tb = B[l.tops[1]] if len(l.tops) > 1 else None
            if any(x.esize != 4 for x in (sb, db, ib)) or rb.cstride < rb.coffset + 8 or (tb is not None and tb.cstride < tb.coffset + 4):
                raise NotImplementedError("layer %s: a top of Proposal is a channel window that ends inside a 16-byte group" % l.name)
            base = RG.anchors(pp.base_size, pp.ratios, pp.scales).astype(F32).reshape(-1)
            par = L.ProposalParams()
            par.H, par.W, par.A, par.feat_stride = sb.shape[2], sb.shape[3], base.size // 4, pp.feat_stride
            par.pre_nms_topn, par.post_nms_topn, par.min_size, par.nms_thresh = pp.pre_nms_topn, pp.post_nms_topn, pp.min_size, pp.nms_thresh
            par.score_cstride, par.score_coffset, par.delta_cstride, par.delta_coffset = sb.cstride, sb.coffset, db.cstride, db.coffset
            par.rois_cstride, par.rois_coffset = rb.cstride, rb.coffset
            par.top_score_cstride, par.top_score_coffset = (tb.cstride, tb.coffset) if tb is not None else (0, 0)
            for i, v in enumerate(base):
                par.anchors[i] = float(v)
            nbytes = int(lib.fcn_proposal_workspace_bytes(C.byref(par)))
            if nbytes <= 0:
                L.check(lib.fcn_proposal_f32(None, None, None, C.byref(par), None, None, None, None, 0, None))      # (raises with the library's text)
                raise RuntimeError("layer %s: Proposal has no plan" % l.name)
            ws, cnt = DeviceBuffer(nbytes, zero=True), DeviceBuffer(16, zero=True)
            self.roi_counts[l.name], self._roi_caps[l.name] = cnt, pp.post_nms_topn
            self._keep.extend([ws, par])
            m, k = par.H * par.W * par.A, min(pp.pre_nms_topn, par.H * par.W * par.A)
            run = lambda st: L.check(lib.fcn_proposal_f32(sb.buf.ptr, db.buf.ptr, ib.ptr, C.byref(par), rb.buf.ptr, tb.buf.ptr if tb is not None else None,
                                                          cnt.ptr, ws.ptr, nbytes, st))
            return [OpTask(l, [Op("proposal", l.name, run, 30.0 * m + 2.0 * m * m + 20.0 * k * k / 2, 24.0 * m + 8.0 * m * ((m + 255) // 256) + k * k / 4.0)],
                           reads=[self._range(b) for b in l.bottoms], writes=[self._range(tp) for tp in l.tops])]
        xb, rb, yb = B[l.bottoms[0]], B[l.bottoms[1]], B[l.tops[0]]
        if any(x.esize != 4 for x in (xb, rb, yb)) or yb.cstride < yb.coffset + _r4(yb.channels):
            raise NotImplementedError("layer %s: the top %s is a channel window that ends inside a 16-byte group" % (l.name, l.tops[0]))
        n, c, h, w = xb.nchw
        r = rb.shape[0]
        if t == "ROIPooling":
            rp = RG.roi_pool_params(l)
            run = lambda st: L.check(lib.fcn_roi_pool_fwd_f32(xb.buf.ptr, rb.buf.ptr, yb.buf.ptr, None, n, h, w, c, xb.cstride, xb.coffset, r, rb.cstride,
                                                              rb.coffset, rp.pooled_h, rp.pooled_w, rp.spatial_scale, yb.cstride, yb.coffset, st))
            return [OpTask(l, [Op("roi_pool", l.name, run, 0.0, 4.0 * (n * h * w * c + r * rp.pooled_h * rp.pooled_w * c))],
                           reads=[self._range(b) for b in l.bottoms], writes=[self._range(l.tops[0])])]
        if t == "PSROIPooling":
            sp = RG.psroi_pool_params(l)
            RG.psroi_pool_shape(l, [self.shapes[b] for b in l.bottoms])
            run = lambda st: L.check(lib.fcn_psroi_pool_fwd_f32(xb.buf.ptr, rb.buf.ptr, yb.buf.ptr, n, h, w, c, xb.cstride, xb.coffset, r, rb.cstride,
                                                                rb.coffset, sp.output_dim, sp.group_size, sp.spatial_scale, yb.cstride, yb.coffset, st))
            return [OpTask(l, [Op("psroi_pool", l.name, run, 1.0 * r * c * 4, 4.0 * (n * h * w * c + r * c))],
                           reads=[self._range(b) for b in l.bottoms], writes=[self._range(l.tops[0])])]
        raise NotImplementedError("layer type %r (layer %s) has no forward kernel yet" % (t, l.name))

    def _download_counts(self, stream: Optional[int]) -> None:
        """The Proposal layers' row counts to the host, enqueued behind the layers (and behind the graph that holds them)."""
        for name, cnt in self.roi_counts.items():
            host = self._roi_count_host.get(name)
            if host is None:
                host = self._roi_count_host[name] = PinnedArray((4,))
            L.check(L.load().fcn_memcpy_d2h_async(host.array.ctypes.data, cnt.ptr, 4, stream))

    def _roi_count(self, name: str) -> int:
        """How many rows the Proposal layer `name` found in the last forward (copied now if that forward left the count on the device)."""
        if not self._counts_valid:
            with self.lock:
                self._download_counts(self.stream)
                L.call("fcn_stream_sync", self.stream)
                self._counts_valid = True
        return min(max(int(self._roi_count_host[name].array.view(np.int32)[0]), 0), self._roi_caps[name])

    def _cut_rois(self, name: str, a: np.ndarray) -> np.ndarray:
        """A blob on the ROI axis of a Proposal as Caffe would shape it: the rows the last forward found."""
        if name not in self.spec.roi_blobs or not getattr(self, "_ran", False):
            return a
        return a[:self._roi_count(self.spec.roi_blobs[name].name)]

    def _compose_detections(self, name: str) -> np.ndarray:
        """Caffe's top of a DetectionOutput from the downloaded buffer (rows, then the count): composed on the host, nothing waits here."""
        raw = self.blobs[name].host
        cap = self.detections[name]
        count = int(raw[7 * cap:7 * cap + 1].view(np.int32)[0])
        l = self.spec.detection_blobs[name]
        return SSD.compose_detections(raw, min(max(count, 0), cap), self.shapes[l.bottoms[0]][0])

    def _dwconv_task(self, li: int, l: Layer, skip: set) -> OpTask:
        """A depthwise Convolution (NetSpec.is_depthwise): one pure launch of csrc/dwconv.hip on the tap-major bank, never a ConvTask -
        it stays out of the grouped launches and the tuner.  An in-place ReLU behind the layer rides in the epilogue.  In the
        half-float engine the bottom holds halves and the top halves or float32; the bank and the bias are float32 in both."""
        lib = L.load()
        g = self._dwgeom(l)
        xb, yb = self.blobs[l.bottoms[0]], self.blobs[l.tops[0]]
        eps = 16 // xb.esize
        if xb.coffset % eps or xb.cstride % eps:
            raise NotImplementedError("depthwise Convolution %s: input view is not 16-byte aligned" % l.name)
        if xb.esize == 4 and yb.esize != 4:
            raise NotImplementedError("f16 engine: depthwise Convolution %s reads the float32 blob %s and writes halves" % (l.name, l.bottoms[0]))
        relu = self._relu_after(li, l, skip)      # (the ReLU half of _fused_after: fcn_dwconv_desc has no second output for a Sigmoid)
        self._conv_layer_meta[l.name] = dict(relu=relu, sigmoid_top=None)
        pd = self.params_dev[l.name]
        flags = (L.CONV_RELU if relu else 0) | (L.CONV_OUT_F32 if xb.esize == 2 and yb.esize == 4 else 0)
        d = dwconv_desc(xb, yb, g, pd[0].ptr, pd[1].ptr if len(pd) > 1 else None, flags)
        fn = lib.fcn_dwconv2d_fwd_f16 if xb.esize == 2 else lib.fcn_dwconv2d_fwd_f32
        op = Op("dwconv", "%s [%dx%d]" % (l.name, g.kh, g.kw), lambda st: L.check(fn(C.byref(d), -1, st)), g.flops, g.bytes)
        return OpTask(l, [op], reads=[self._range(l.bottoms[0])], writes=[self._range(l.tops[0])], dwconv=d)

    def _rconv_task(self, li: int, l: Layer, skip: set) -> OpTask:
        """A Convolution whose axes differ in kernel, pad or stride (dilated or not), or a square one with dilation > 1 (the case with
        equal axes): a problem of csrc/rconv.hip, never of the tiled family or the tuner.  The bank is the layer's parameter blob where
        it lies; an in-place ReLU behind the layer rides in the epilogue.  In a half-float engine whose NetSpec was built with
        rconv_f16=True the bottom and the bank hold halves, the bias is float32 and the top holds halves or float32 (a net output);
        without the keyword a half-float engine refuses the layer."""
        rect, dil, ng = is_rectangular(l), layer_dilation(l), self._conv_groups(l)
        who = "rectangular Convolution %s (%dx%d stride %dx%d pad %dx%d)" % (l.name, *layer_geometry(l)) if rect else \
            "Convolution %s with dilation %d" % (l.name, dil)
        if self.f16 and not self.spec.rconv_f16:
            raise NotImplementedError("f16 engine: %s has no half-float kernel" % who)
        if ng > 1:
            raise NotImplementedError("%s: group %d" % (who, ng) if rect else "Convolution %s: group %d together with dilation %d" % (l.name, ng, dil))
        g = self._rgeom(l)
        xb, yb = self.blobs[l.bottoms[0]], self.blobs[l.tops[0]]
        if self.f16 and xb.esize == 4:
            raise NotImplementedError("f16 engine: %s reads the float32 blob %s" % (who, l.bottoms[0]))
        eps = 16 // xb.esize
        if xb.coffset % eps or xb.cstride % eps:
            raise NotImplementedError("%s Convolution %s: input view is not 16-byte aligned" % ("rectangular" if rect else "dilated", l.name))
        relu = self._relu_after(li, l, skip)      # (the ReLU half of _fused_after: fcn_rconv_desc has no second output for a Sigmoid)
        self._conv_layer_meta[l.name] = dict(relu=relu, sigmoid_top=None)
        pd = self.params_dev[l.name]
        flags = (L.CONV_RELU if relu else 0) | (L.CONV_OUT_F32 if xb.esize == 2 and yb.esize == 4 else 0)
        d = rconv_desc(xb, yb, g, pd[0].ptr, pd[1].ptr if len(pd) > 1 else None, flags)
        return OpTask(l, [], reads=[self._range(l.bottoms[0])], writes=[self._range(l.tops[0])], rconv=d)

    def _emit_rconvs(self, items: List[OpTask]) -> None:
        """The dilated and rectangular convolutions of one level: the square dilated ones that read the same bottom (the four branches
        of an ASPP head) share ONE fcn_rconv2d_prepare plan and launch, op kind "dconv", the label shows the dilations; so do the
        rectangular ones (the 1x3 / 3x1 pair of an 8-grid Inception module), op kind "rconv", the label shows the kernels.  Square
        launches come first.  FLOPs are booked as 2 N OH OW Cin Cout kh kw.  A half-float engine prepares and launches through
        fcn_rconv2d_prepare_f16 / fcn_rconv2d_f16 and books its halves as 2 bytes."""
        lib = L.load()
        prepare, fn = ("fcn_rconv2d_prepare_f16", lib.fcn_rconv2d_f16) if self.f16 else ("fcn_rconv2d_prepare", lib.fcn_rconv2d_f32)
        groups: Dict[Tuple[bool, Range], List[OpTask]] = {}
        for it in items:
            groups.setdefault((is_rectangular(it.layer), it.reads[0]), []).append(it)
        for (rect, _), chunk in sorted(groups.items(), key=lambda kv: kv[0][0]):
            arr = (L.RConvDesc * len(chunk))(*[it.rconv for it in chunk])
            ws = DeviceBuffer(int(lib.fcn_rconv2d_workspace_bytes(arr, len(chunk))), zero=False)
            plan = L.RConvPlan()
            L.call(prepare, arr, len(chunk), ws.ptr, -1, C.byref(plan))
            self._keep.extend([arr, ws, plan])
            geoms = [self._rgeom(it.layer) for it in chunk]
            shows = ",".join("%dx%d" % (g.kh, g.kw) for g in geoms) if rect else "d" + ",".join(str(g.d) for g in geoms)
            label = "%s [%s %dwg]" % ("+".join(it.layer.name for it in chunk), shows, plan.total_tiles)
            byts = sum(g.bytes for g in geoms)
            if self.f16:
                byts = sum(g.bytes_as(self.blobs[it.layer.bottoms[0]].esize, self.blobs[it.layer.tops[0]].esize) for g, it in zip(geoms, chunk))
            self.ops.append(Op("rconv" if rect else "dconv", label, lambda st, p=plan: L.check(fn(C.byref(p), st)),
                               sum(g.flops for g in geoms), byts))

    def _emit_group(self, chunk: List[ConvTask], fused: List[OpTask], tail: Optional[dict]) -> None:
        """One grouped launch of `chunk` (at most 16 convolutions of one level); `fused` MAX poolings ride in it."""
        lib = L.load()
        name = "+".join(it.layer.name for it in chunk)
        flops = sum(it.flops for it in chunk)
        byts = sum(it.bytes for it in chunk)
        arr = (L.ConvDesc * len(chunk))(*[it.desc for it in chunk])
        ws = DeviceBuffer(int(lib.fcn_conv2d_group_workspace_bytes(len(chunk))), zero=False)
        self._group_workspaces.append(ws)
        grp = L.ConvGroup()
        parr = (L.PoolDesc * max(len(fused), 1))(*[pt.pool_desc for pt in fused])
        tune_key = name + ("{+%d pool}" % len(fused) if fused else "")
        tailed = tail is not None and any(id(it) in tail["producers"] for it in chunk)
        if tailed:      # this launch writes (part of) the blob the narrow heads read: it carries them as its tail
            fin = 1 if any(tail["producers"][id(it)] == tail["final_level"] for it in chunk if id(it) in tail["producers"]) else 0
            tail["desc"].finalize = fin
            L.call("fcn_conv2d_group_attach_tail", ws.ptr, C.byref(tail["desc"]))
            tune_key += "{+tail%d}" % fin
            if fin:
                flops += sum(ht.flops for ht in tail["heads"])
                byts += sum(4.0 * ht.desc.Cout * (ht.desc.N * ht.desc.OH * ht.desc.OW + ht.desc.Cin) for ht in tail["heads"])
        cfg = self.tuner.conv_cfg(tune_key, arr, len(chunk), ws, parr, len(fused)) if self.autotune else -1
        L.call("fcn_conv2d_group_prepare_fused", arr, len(chunk), parr, len(fused), ws.ptr, cfg, C.byref(grp))
        self._keep.extend([arr, parr, ws, grp])
        kind = "conv_group" if len(chunk) > 1 else "conv"
        label = "%s [cfg%d %dwg]" % (name, grp.cfg, grp.total_tiles)
        if fused:
            label = "%s {+%s}" % (label, "+".join(pt.layer.name for pt in fused))
            byts += sum(pt.ops[0].bytes for pt in fused)
        if tailed:
            label = "%s {%s %s}" % (label, "tail:" if tail["desc"].finalize else "partial sums of", "+".join(ht.layer.name for ht in tail["heads"]))
        self.ops.append(Op(kind, label, lambda st, g=grp: L.check(lib.fcn_conv2d_fwd_group_f32(C.byref(g), st)), flops, byts))

    def _emit_convs(self, items: List[ConvTask], pools: List[OpTask], tail: Optional[dict]) -> None:
        """One grouped launch per 16 convolutions of a level; the level's fusable MAX poolings ride in the first one.  Half-float
        engines may cut a level in two launches - its 3x3 / 5x5 convolutions and its 1x1 convolutions - when the autotuner
        finds the pair faster (the streaming kernel's configurations are shaped for one kind or the other)."""
        for base in range(0, len(items), 16):
            chunk = items[base:base + 16]
            fused = pools[:2] if base == 0 and len(chunk) <= 8 else []
            parts = [chunk]
            if self.f16 and self.autotune and not fused and len(chunk) > 1:
                parts = self.tuner.split_level(chunk)
            for part in parts:
                self._emit_group(part, fused, tail)
                fused = []
            if base == 0 and len(chunk) <= 8:
                del pools[:2]
        for pt in pools:            # no convolution launch at this level to ride in
            self.ops.extend(pt.ops)
        pools.clear()

    def _emit_score_ops(self) -> None:
        """Solver::Test's `test_score[idx] += result`, on the device: one accumulator per output blob (NCHW order, float32) and one
        fcn_score_accumulate_f32 launch per blob behind the last layer, inside whatever graph the forward is captured into."""
        lib = L.load()
        for nm in self.outputs:
            b = self.blobs[nm]
            if b.esize != 4 or b.lazy_shift:
                raise NotImplementedError("score_outputs: output blob %s is not a plain float32 blob" % nm)
            count = int(np.prod(b.shape)) if b.shape else 1
            acc = DeviceBuffer(max(4 * count, 16), zero=True)
            self.score_acc[nm] = acc
            if b.nchw is not None:
                n, c, h, w = b.nchw
                args = (acc.ptr, b.buf.ptr, n, h * w, c, b.cstride, b.coffset)
            else:
                args = (acc.ptr, b.ptr, 1, 1, count, count, 0)
            self.ops.append(Op("score", "score:" + nm, lambda st, a=args: L.check(lib.fcn_score_accumulate_f32(*a, st)), 0.0, 12.0 * count))

    def _plan_tail(self, tasks: List[Task], levels: List[int]) -> Optional[dict]:
        """The detection heads (cvg/classifier + bbox/regressor of models/deploy.prototxt: 4 + 16 outputs over inception_5b/output) as the
        TAIL of the launches that produce their input (fcn_conv2d_group_attach_tail, csrc/conv_common.h): as a launch of their own they are
        0.03 GFLOP behind a whole launch's fixed cost (6 us of a 266 us frame).  Taken when the net's LAST convolution level holds only
        narrow float32 1x1 problems over one blob whose channels are all written by bias + ReLU convolutions of the one or two levels
        before, in whole 32-channel groups.  Returns None (heads launched as before) or the plan emit_group() works from."""
        if self.f16 or self.spec.phase != "TEST" or not (self.fuse and self.group_convs) or os.environ.get("FCN_CONV_TAIL", "0") != "1":
            return None
        conv_idx = [i for i, t in enumerate(tasks) if isinstance(t, ConvTask)]
        if not conv_idx:
            return None
        lh = max(levels[i] for i in conv_idx)
        heads = [i for i in conv_idx if levels[i] == lh]
        if any(levels[i] >= lh for i, t in enumerate(tasks) if not isinstance(t, ConvTask)) or not 1 <= len(heads) <= 4:
            return None
        d0 = tasks[heads[0]].desc
        m = d0.N * d0.OH * d0.OW
        rows = 0
        for i in heads:
            d = tasks[i].desc
            if (d.kh, d.kw, d.stride, d.pad) != (1, 1, 1, 0) or d.x != d0.x or d.x_cstride != d0.x_cstride or d.Cin != d0.Cin or d.Cin % 32 or d.Cin > 1024 or d.Cout % 4 \
                    or (d.flags & ~(L.CONV_RELU | L.CONV_SIGMOID2)) or d.y_cstride % 4 or d.y_coffset % 4 or (d.y2 and (d.y2_cstride % 4 or d.y2_coffset % 4)):
                return None
            rows += d.Cout
        if rows > 24 or m > 4096:      # (scratch: K / 32 x M x rows floats)
            return None
        xr = tasks[heads[0]].reads
        producers: Dict[int, int] = {}
        covered = 0
        for i, t in enumerate(tasks):
            if i in heads or not ranges_hit(t.writes, xr):
                continue
            if not isinstance(t, ConvTask):
                return None
            d = t.desc
            if levels[i] not in (lh - 1, lh - 2) or d.y != d0.x or d.y_cstride != d0.x_cstride or d.N * d.OH * d.OW != m \
                    or d.Cout % 32 or d.y_coffset % 32 or d.y_coffset + d.Cout > d0.Cin or (d.flags & ~L.CONV_RELU) or d.y_cstride % 4:
                return None
            producers[id(t)] = levels[i]
            covered += d.Cout
        if covered != d0.Cin or not producers:
            return None
        for lv in set(producers.values()):      # each producing level is ONE launch
            if sum(1 for i in conv_idx if levels[i] == lv) > 8:
                return None
        # (other readers of the blob - none in the reference's nets - still see it complete: every producer stores its own output as before)
        lib = L.load()
        desc = L.ConvTail()
        desc.n = len(heads)
        for j, i in enumerate(heads):
            desc.heads[j] = tasks[i].desc
        sb, ab = int(lib.fcn_conv2d_tail_scratch_bytes(C.byref(desc))), int(lib.fcn_conv2d_tail_arrive_bytes(C.byref(desc)))
        if sb <= 0 or ab <= 0:
            return None
        scratch, arrive = DeviceBuffer(sb, zero=False), DeviceBuffer(ab, zero=True)
        desc.scratch, desc.arrive = scratch.ptr, arrive.ptr
        self._keep.extend([scratch, arrive, desc])
        return dict(desc=desc, heads=[tasks[i] for i in heads], producers=producers, final_level=max(producers.values()))

    def _fuse_pool_lrn(self, tasks: List[Task]) -> List[Task]:
        """MAX pooling directly followed by LRN (pool1 -> norm1) or LRN directly followed by MAX pooling (norm2 -> pool2)
        become ONE launch that never writes the blob between them (inference engines; fcn_maxpool_lrn5_fwd_f32).  The
        blob in the middle stays readable: read_blob() runs the first layer on its own when somebody asks for it."""
        B, lib = self.blobs, L.load()
        out: List[Task] = []
        i = 0
        while i < len(tasks):
            a = tasks[i]
            b = tasks[i + 1] if i + 1 < len(tasks) else None
            op = None
            if isinstance(a, OpTask) and isinstance(b, OpTask):
                la, lb = a.layer, b.layer
                if {la.type, lb.type} == {"Pooling", "LRN"} and len(la.tops) == 1 and lb.bottoms == [la.tops[0]] and la.tops[0] != la.bottoms[0]:
                    op = self._pool_lrn_op(la, lb)
            if op is None:
                out.append(a)
                i += 1
                continue
            self._lazy_blob_ops[a.layer.tops[0]] = list(a.ops)
            c = tasks[i + 2] if i + 2 < len(tasks) else None
            op3 = self._pool_lrn_conv_op(a.layer, b.layer, c) if isinstance(c, ConvTask) else None
            if op3 is not None:      # ... -> 1x1 convolution in the same launch: the normalised blob is not written either
                self._lazy_blob_ops[b.layer.tops[0]] = [op]
                out.append(OpTask(c.layer, [op3], reads=a.reads, writes=c.writes))
                i += 3
                continue
            out.append(OpTask(b.layer, [op], reads=a.reads, writes=b.writes))
            i += 2
        return out

    def _pool_lrn_conv_op(self, la: Layer, lb: Layer, ct: ConvTask) -> Optional[Op]:
        """MAX pooling -> LRN -> 1x1 convolution (+ in-place ReLU) as one launch (fcn_maxpool_lrn5_conv1x1_fwd_f32: deploy.prototxt's
        pool1/3x3_s2 -> pool1/norm1 -> conv2/3x3_reduce): as a launch of its own that convolution is two chunks of K behind a whole
        launch's fixed cost.  The FLOPs of the convolution are booked on this op (kind "pool_lrn_conv")."""
        if os.environ.get("FCN_FUSE_POOL_LRN_CONV", "1") == "0" or la.type != "Pooling":
            return None
        B, lib = self.blobs, L.load()
        lc, d = ct.layer, ct.desc
        mid = lb.tops[0]
        if lc.bottoms != [mid] or [q.name for q in self.consumers.get(mid, [])] != [lc.name] or len(self.producers.get(mid, [])) != 1 \
                or mid in self.outputs or mid in self.alias:
            return None
        xb, nb = B[la.bottoms[0]], B[mid]
        k, s, pad = kernel_stride_pad(la.sub("pooling_param"))
        lp = lb.sub("lrn_param")
        esz = xb.esize
        want = (L.CONV_F16 if esz == 2 else 0)
        if (d.kh, d.kw, d.stride, d.pad) != (1, 1, 1, 0) or d.Cin != 64 or d.Cout != 64 or xb.channels != 64 or k != 3 or nb.esize != esz \
                or (d.flags & ~L.CONV_RELU) != want or d.in_shift != 0.0 or nb.coffset or d.y_cstride % (16 // esz) or d.y_coffset % (16 // esz) or B[lc.tops[0]].esize != esz:
            return None
        n, c, h, w = xb.shape
        oh, ow = d.OH, d.OW
        if (oh + 3) // 4 > 65535 or n > 65535:
            return None
        # halves: the LDS-patch form only (3 x 3 / stride 2 / unpadded), and only where that form is the one the two-layer launch takes (large blobs)
        if esz == 2 and ((s, pad) != (2, 0) or n * c * h * w < 1 << 22):
            return None
        al, be, kk = float(lp.get("alpha", 1.0)), float(lp.get("beta", 0.75)), float(lp.get("k", 1.0))
        relu = 1 if d.flags & L.CONV_RELU else 0
        fn = lib.fcn_maxpool_lrn5_conv1x1_fwd_f16 if esz == 2 else lib.fcn_maxpool_lrn5_conv1x1_fwd_f32
        return Op("pool_lrn_conv", "%s+%s+%s" % (la.name, lb.name, lc.name), lambda st: L.check(fn(
            xb.ptr, n, h, w, c, xb.cstride, k, s, pad, oh, ow, al, be, kk, d.w, d.bias, d.Cout, relu, d.y, d.y_cstride, d.y_coffset, st)),
            ct.flops, float(esz) * (xb.pixels * c + n * oh * ow * d.Cout))

    def _pool_lrn_op(self, la: Layer, lb: Layer) -> Optional[Op]:
        B, lib = self.blobs, L.load()
        pool, lrn = (la, lb) if la.type == "Pooling" else (lb, la)
        if len(pool.tops) != 1:      # a pooling with a mask top: the fused launches write no argmax
            return None
        mid = la.tops[0]
        if [q.name for q in self.consumers.get(mid, [])] != [lb.name] or len(self.producers.get(mid, [])) != 1 or mid in self.outputs:
            return None
        pp, lp = pool.sub("pooling_param"), lrn.sub("lrn_param")
        if str(pp.get("pool", "MAX")) != "MAX" or bool(pp.get("global_pooling", False)):
            return None
        if str(lp.get("norm_region", "ACROSS_CHANNELS")) != "ACROSS_CHANNELS" or int(lp.get("local_size", 5)) != 5:
            return None
        xb, mb, yb = B[la.bottoms[0]], B[mid], B[lb.tops[0]]
        esz = xb.esize
        eps = 16 // esz      # elements per 16-byte channel group: 4 floats or 8 halves
        if any(t.esize != esz or t.coffset or t.cstride % eps for t in (xb, mb, yb)) or xb.channels % eps or mid in self.alias or lb.tops[0] in self.alias:
            return None
        n, c, h, w = xb.shape
        _, _, oh, ow = yb.shape
        k, s, pad = kernel_stride_pad(pp)
        if pad >= k or max((h + 7) // 8, n) > 65535:
            return None
        # Measured on MI355X: the single pass saves a launch and the round trip of the blob in the middle (batch 1: 9.1 -> 7.1
        # and 11.1 -> 8.2 us) but recomputes the neighbour groups' maxima / the normalisation per window element; once the
        # blobs are tens of MB the two bandwidth-bound launches are as fast or faster (batch-32 halves: 73 -> 88 and 103 -> 102 us)
        # (half-float 3x3 / stride 2 poolings of at most 192 channels take the LDS-patch kernel at those sizes - round 3: LRN once
        #  per pixel, the blob in between never written: norm2 + pool2 104 -> ~45 us at batch 32)
        if n * c * h * w > 8 << 20 and not (esz == 2 and (k, s, pad) == (3, 2, 0) and c <= 192):
            return None
        al, be, kk = float(lp.get("alpha", 1.0)), float(lp.get("beta", 0.75)), float(lp.get("k", 1.0))
        first = 1 if la.type == "LRN" else 0
        fn = lib.fcn_maxpool_lrn5_fwd_f16 if esz == 2 else lib.fcn_maxpool_lrn5_fwd_f32
        return Op("pool_lrn", "%s+%s" % (la.name, lb.name), lambda st: L.check(fn(
            xb.ptr, yb.ptr, n, h, w, c, xb.cstride, k, s, pad, oh, ow, yb.cstride, first, al, be, kk, st)),
            0.0, float(esz) * (xb.pixels * c + yb.pixels * c))

    def _fusable_pool_desc(self, l: Layer) -> Optional[L.PoolDesc]:
        if os.environ.get("FCN_FUSE_POOLS", "1") == "0":      # (experiments: pools as launches of their own)
            return None
        # Measured on MI355X: riding in the convolution launch saves a launch (what counts at batch 1-8: 2520 vs 2270
        # frames/s at batch 1) but the pool workgroups are shaped by the convolution's tile; on the half-float batch-32
        # path the dedicated 8-channels-per-lane kernel is faster than its share of the fused launch (forward 2.11 -> 2.02 ms).
        xb = self.blobs.get(l.bottoms[0])
        if self.f16 and xb is not None and xb.pixels >= 16384:
            return None
        if self.f16 and len(l.tops) == 2:      # a masked pooling of halves: fcn_maxpool_idx_fwd_f16
            return None
        return self._fusable_pool_desc_impl(l)

    def _fusable_pool_desc_impl(self, l: Layer) -> Optional[L.PoolDesc]:
        """fcn_pool_desc of a MAX pooling that can ride in a convolution launch (16-byte channel groups), else None."""
        if l.type != "Pooling":
            return None
        pp = l.sub("pooling_param")
        if str(pp.get("pool", "MAX")) != "MAX" or bool(pp.get("global_pooling", False)):
            return None
        xb, yb = self.blobs[l.bottoms[0]], self.blobs[l.tops[0]]
        n, c, h, w = xb.shape
        _, _, oh, ow = yb.shape
        k, s, pad = kernel_stride_pad(pp)
        eps = 16 // xb.esize
        if xb.esize != yb.esize or (xb.esize == 2 and self.spec.phase != "TEST"):
            return None
        if c % eps or xb.cstride % eps or yb.cstride % eps or yb.coffset % eps or xb.coffset % eps or n * oh * ow * (c // eps) >= 1 << 30:
            return None
        idx = self.aux_dev.get(l.name)
        d = L.PoolDesc()
        d.x, d.y, d.idx = xb.ptr, yb.buf.ptr, (idx.ptr if idx is not None else None)
        d.N, d.H, d.W, d.C, d.x_cstride, d.k, d.stride, d.pad = n, h, w, c, xb.cstride, k, s, pad
        d.OH, d.OW, d.y_cstride, d.y_coffset = oh, ow, yb.cstride, yb.coffset
        d.f16 = 1 if xb.esize == 2 else 0
        return d

    def _loss_grad_ptr(self, blob: str) -> Optional[int]:
        """Device address the loss kernel writes d(loss)/d(blob) to; None in an inference engine."""
        return None

    def _emit_simple(self, l: Layer) -> List[Op]:
        """The launches of one layer that is not a convolution."""
        B, t = self.blobs, l.type
        halves = [b for b in list(l.bottoms) + list(l.tops) if b in B and B[b].esize == 2]
        acts = ACT_TYPES if self.spec.activations else ()      # (csrc/act.hip: only a NetSpec built with activations=True has them)
        if halves and t not in ("Pooling", "LRN", "Eltwise", "Softmax", "Deconvolution", "Dropout", "Concat", "Slice", "Crop", "ReLU", "Interp", "Upsample") + acts + NEURON_TYPES + SHUFFLE_TYPES:
            raise NotImplementedError("f16 engine: layer type %s (%s) has no half-float kernel" % (t, l.name))
        if t in acts:
            return self._fwd_act(l, halves)
        if t in NEURON_TYPES:
            return self._fwd_neuron(l, halves)
        if t in SHUFFLE_TYPES:
            return self._fwd_shuffle(l, halves)
        emit = {"Pooling": self._fwd_pooling, "LRN": self._fwd_lrn, "ReLU": self._fwd_pointwise, "Sigmoid": self._fwd_pointwise,
                "Power": self._fwd_pointwise, "Dropout": self._fwd_dropout, "L1Loss": self._fwd_loss, "EuclideanLoss": self._fwd_loss,
                "Softmax": self._fwd_softmax, "SoftmaxWithLoss": self._fwd_softmax_loss, "Accuracy": self._fwd_accuracy,
                "Slice": self._fwd_slice, "Concat": self._fwd_concat, "Eltwise": self._fwd_eltwise,
                "Deconvolution": self._fwd_deconvolution, "Crop": self._fwd_crop, "Interp": self._fwd_interp,
                "Upsample": self._fwd_upsample}.get(t)
        if emit is None:
            raise NotImplementedError("layer type %r (layer %s) has no forward kernel yet" % (t, l.name))
        return emit(l, halves)

    def _copy_op(self, name: str, sb: Blob, so: int, db: Blob, do: int, pixels: int, c: int) -> Op:
        """`c` channels of every pixel from channel `so` of sb's buffer to channel `do` of db's (Dropout at TEST, copied Concat / Slice)."""
        if sb.esize != db.esize:
            raise NotImplementedError("f16 engine: %s copies between half and float32 blobs" % name)
        lib = L.load()
        fn = lib.fcn_copy_channels_f16 if sb.esize == 2 else lib.fcn_copy_channels_f32
        return Op("copy", name, lambda st: L.check(fn(sb.buf.ptr, db.buf.ptr, pixels, c, sb.cstride, so, db.cstride, do, st)),
                  0.0, 2.0 * sb.esize * pixels * c)

    def _fwd_crop(self, l: Layer, halves: List[str]) -> List[Op]:
        """Crop: the window of bottom 0 at crop_param's offsets, in the size of bottom 1 - which lends its shape and is never read."""
        lib = L.load()
        xb, yb = self.blobs[l.bottoms[0]], self.blobs[l.tops[0]]
        if xb.esize != yb.esize and not (xb.esize == 2 and yb.esize == 4):      # (halves into a float32 net output: the converting kernel)
            raise NotImplementedError("f16 engine: Crop %s copies between half and float32 blobs" % l.name)
        _, (_, oc, oy, ox) = crop_window(l, xb.shape, self.blobs[l.bottoms[1]].shape)
        n, _, h, w = xb.shape
        _, c, oh, ow = yb.shape
        fn = lib.fcn_crop_fwd_f32 if xb.esize == 4 else lib.fcn_crop_fwd_f16 if yb.esize == 2 else lib.fcn_crop_fwd_f16_f32
        return [Op("crop", l.name, lambda st: L.check(fn(xb.buf.ptr, yb.buf.ptr, n, h, w, c, xb.cstride, xb.coffset + oc, oy, ox, oh, ow,
                                                         yb.cstride, yb.coffset, st)), 0.0, float(xb.esize + yb.esize) * yb.pixels * c)]

    def _fwd_interp(self, l: Layer, halves: List[str]) -> List[Op]:
        """Interp: bilinear resampling of the bottom's effective window (interp_param's pads crop) to the top's size.  Halves are read
        as halves and stored as halves or - a net's output - as float32."""
        lib = L.load()
        xb, yb = self.blobs[l.bottoms[0]], self.blobs[l.tops[0]]
        if xb.esize == 4 and yb.esize == 2:
            raise NotImplementedError("f16 engine: Interp %s reads the float32 blob %s and writes halves" % (l.name, l.bottoms[0]))
        n, c, h, w = xb.shape
        oh, ow, pad_beg, pad_end = interp_size(l, h, w)
        byts = float(xb.esize) * n * (h + pad_beg + pad_end) * (w + pad_beg + pad_end) * c + float(yb.esize) * yb.pixels * c
        if xb.esize == 2:
            out_f32 = 1 if yb.esize == 4 else 0
            run = lambda st: L.check(lib.fcn_interp_fwd_f16(xb.buf.ptr, yb.buf.ptr, n, h, w, c, xb.cstride, xb.coffset, pad_beg, pad_end, oh, ow,
                                                            yb.cstride, yb.coffset, out_f32, st))
        else:
            run = lambda st: L.check(lib.fcn_interp_fwd_f32(xb.buf.ptr, yb.buf.ptr, n, h, w, c, xb.cstride, xb.coffset, pad_beg, pad_end, oh, ow,
                                                            yb.cstride, yb.coffset, st))
        return [Op("interp", l.name, run, 0.0, byts)]

    def _fwd_upsample(self, l: Layer, halves: List[str]) -> List[Op]:
        """Upsample: bottom 0 scattered to the pixels that the mask names - the argmax buffer of the MAX pooling whose second top the mask
        is - as a gather over the top; everything else in the top is zero.  Halves are read as halves and stored as halves or - a net's
        output - as float32; the argmax is int32 in both engines."""
        lib = L.load()
        xb, yb = self.blobs[l.bottoms[0]], self.blobs[l.tops[0]]
        pool = self.spec.mask_blobs[l.bottoms[1]]
        idx = self.aux_dev[pool.name]
        if xb.esize == 4 and yb.esize == 2:
            raise NotImplementedError("f16 engine: Upsample %s reads the float32 blob %s and writes halves" % (l.name, l.bottoms[0]))
        k, s, pad = kernel_stride_pad(pool.sub("pooling_param"))
        n, c, ph, pw = xb.shape
        _, _, h, w = yb.shape
        byts = float(xb.esize + 4) * xb.pixels * c + float(yb.esize) * yb.pixels * c
        if xb.esize == 2:
            out_f32 = 1 if yb.esize == 4 else 0
            run = lambda st: L.check(lib.fcn_unpool_fwd_f16(xb.buf.ptr, idx.ptr, yb.buf.ptr, n, ph, pw, c, xb.cstride, xb.coffset, k, s, pad, h, w,
                                                            yb.cstride, yb.coffset, out_f32, st))
        else:
            run = lambda st: L.check(lib.fcn_unpool_fwd_f32(xb.buf.ptr, idx.ptr, yb.buf.ptr, n, ph, pw, c, xb.cstride, xb.coffset, k, s, pad, h, w,
                                                            yb.cstride, yb.coffset, st))
        return [Op("unpool", l.name, run, 0.0, byts)]

    def _fwd_pooling(self, l: Layer, halves: List[str]) -> List[Op]:
        lib = L.load()
        xb, yb = self.blobs[l.bottoms[0]], self.blobs[l.tops[0]]
        pp = l.sub("pooling_param")
        g = self._geom(l, (xb.shape[2], 1, 0) if bool(pp.get("global_pooling", False)) else None)
        c = g.cin
        byts = float(xb.esize) * (xb.pixels * c + yb.pixels * c)
        is_max = str(pp.get("pool", "MAX")) == "MAX"
        masked = len(l.tops) == 2      # (netspec: MAX only) the argmax is the mask blob: kept in TEST too, and written by the half engine
        if halves and (xb.esize != 2 or yb.esize != 2):
            raise NotImplementedError("f16 engine: pooling %s" % l.name)
        if halves and is_max and c % 8:      # (fcn_maxpool_fwd_f16 / fcn_maxpool_idx_fwd_f16 would refuse at the first forward)
            raise NotImplementedError("f16 engine: MAX pooling %s over %d channels (the half-float kernels take whole 8-channel segments)" % (l.name, c))
        if is_max and (masked or not halves):
            idx_ptr = None
            if masked or self.spec.phase == "TRAIN":      # backward routes the gradient to the argmax; an Upsample scatters by it
                ib = DeviceBuffer(yb.pixels * c * 4, zero=False)
                self.aux_dev[l.name] = ib
                idx_ptr = ib.ptr
                byts += 4.0 * yb.pixels * c if masked else 0.0
            if halves:
                run = lambda st: L.check(lib.fcn_maxpool_idx_fwd_f16(
                    xb.ptr, yb.buf.ptr, idx_ptr, g.n, g.h, g.w, c, xb.cstride, g.k, g.s, g.pad, g.oh, g.ow, yb.cstride, yb.coffset, st))
            else:
                run = lambda st: L.check(lib.fcn_maxpool_fwd_f32(
                    xb.ptr, yb.buf.ptr, idx_ptr, g.n, g.h, g.w, c, xb.cstride, g.k, g.s, g.pad, g.oh, g.ow, yb.cstride, yb.coffset, st))
        else:
            fn = (lib.fcn_maxpool_fwd_f16 if is_max else lib.fcn_avepool_fwd_f16) if halves else lib.fcn_avepool_fwd_f32
            run = lambda st: L.check(fn(
                xb.ptr, yb.buf.ptr, g.n, g.h, g.w, c, xb.cstride, g.k, g.s, g.pad, g.oh, g.ow, yb.cstride, yb.coffset, st))
        return [Op("maxpool" if is_max else "avepool", l.name, run, 0.0, byts)]

    def _fwd_lrn(self, l: Layer, halves: List[str]) -> List[Op]:
        lib = L.load()
        xb, yb = self.blobs[l.bottoms[0]], self.blobs[l.tops[0]]
        p = l.sub("lrn_param")
        if str(p.get("norm_region", "ACROSS_CHANNELS")) != "ACROSS_CHANNELS":
            raise NotImplementedError("LRN WITHIN_CHANNEL")
        if yb.coffset != 0:
            raise NotImplementedError("LRN into a channel slice")
        ls, al, be, kk = int(p.get("local_size", 5)), float(p.get("alpha", 1.0)), float(p.get("beta", 0.75)), float(p.get("k", 1.0))
        scale_ptr = None
        if self.spec.phase == "TRAIN":
            sb = DeviceBuffer(xb.pixels * xb.channels * 4, zero=False)
            self.aux_dev[l.name] = sb
            scale_ptr = sb.ptr
        if halves:
            if xb.esize != 2 or yb.esize != 2 or xb.coffset:
                raise NotImplementedError("f16 engine: LRN %s" % l.name)
            if ls != 5:      # (fcn_lrn_fwd_f16 would refuse at the first forward, inside the graph capture)
                raise NotImplementedError("f16 engine: LRN %s with local_size %d (the half-float kernel takes 5 only)" % (l.name, ls))
            if xb.channels % 8:
                raise NotImplementedError("f16 engine: LRN %s over %d channels (the half-float kernel takes whole 8-channel segments)" % (l.name, xb.channels))
            return [Op("lrn", l.name, lambda st: L.check(lib.fcn_lrn_fwd_f16(
                xb.ptr, yb.ptr, xb.pixels, xb.channels, xb.cstride, yb.cstride, ls, al, be, kk, st)), 0.0, 4.0 * xb.pixels * xb.channels)]
        return [Op("lrn", l.name, lambda st: L.check(lib.fcn_lrn_fwd_f32(
            xb.ptr, yb.ptr, scale_ptr, xb.pixels, xb.channels, xb.cstride, yb.cstride, ls, al, be, kk, st)),
            0.0, 8.0 * xb.pixels * xb.channels)]

    def _fwd_pointwise(self, l: Layer, halves: List[str]) -> List[Op]:
        """ReLU, Sigmoid and Power as layers of their own."""
        lib, t = L.load(), l.type
        xb, yb = self.blobs[l.bottoms[0]], self.blobs[l.tops[0]]
        if halves:
            # a ReLU of its own over halves (on the Eltwise tops of a ResNet): the BatchNorm / Scale apply launch with every operand
            # NULL is y = relu(x), exactly
            if float(l.sub("relu_param").get("negative_slope", 0.0)) != 0.0 or xb.esize != 2 or yb.esize != 2 or xb.nchw is None \
                    or xb.coffset % 8 or yb.coffset % 8:
                raise NotImplementedError("f16 engine: ReLU %s with a negative slope, between half and float32 blobs or on an unaligned window" % l.name)
            pix, c = xb.pixels, xb.channels
            return [Op("relu", l.name, lambda st: L.check(lib.fcn_batchnorm_apply_f16(
                xb.buf.ptr, yb.buf.ptr, pix, c, xb.cstride, xb.coffset, yb.cstride, yb.coffset, None, None, None, 0.0, None, None, 1, st)),
                0.0, 4.0 * pix * c)]
        if not all(b.coffset == 0 and (b.nchw is None or b.cstride == _r4(b.channels)) for b in (xb, yb)):
            # a channel window of another blob's buffer (a Pooling top that a Concat view holds, with its ReLU in place): the flat
            # kernels below run over whole pixels - at offset 0 they would rewrite the neighbours' channels as well.  A plain ReLU
            # takes the BatchNorm / Scale apply launch with every operand NULL, y = relu(x) exactly, which keeps to its window
            plain = t == "ReLU" and float(l.sub("relu_param").get("negative_slope", 0.0)) == 0.0 and self.spec.phase == "TEST"
            if not plain or xb.nchw is None or xb.shape != yb.shape or any(b.coffset % 4 or b.cstride % 4 for b in (xb, yb)):
                raise NotImplementedError("%s on a channel slice (layer %s)" % (t, l.name))
            pix, c = xb.pixels, xb.channels
            return [Op("relu", l.name, lambda st: L.check(lib.fcn_batchnorm_apply_f32(
                xb.buf.ptr, yb.buf.ptr, None, pix, c, xb.cstride, xb.coffset, yb.cstride, yb.coffset, _r4(c), None, None, None, None, 0.0, None, None,
                1, st)), 0.0, 8.0 * pix * c)]
        count = xb.pixels * xb.cstride
        if t == "ReLU":
            ns = float(l.sub("relu_param").get("negative_slope", 0.0))
            fn = lambda st: L.check(lib.fcn_relu_fwd_f32(xb.ptr, yb.ptr, count, ns, st))
        elif t == "Sigmoid":
            fn = lambda st: L.check(lib.fcn_sigmoid_fwd_f32(xb.ptr, yb.ptr, count, st))
        else:
            p = l.sub("power_param")
            pw, sc, sh = float(p.get("power", 1.0)), float(p.get("scale", 1.0)), float(p.get("shift", 0.0))
            fn = lambda st: L.check(lib.fcn_power_fwd_f32(xb.ptr, yb.ptr, count, pw, sc, sh, st))
        return [Op(t.lower(), l.name, fn, 0.0, 8.0 * count)]

    def _chan_group_views(self, l: Layer):
        """(xb, yb, pixels, channels) of a one-bottom layer that runs on csrc/chan_group.h's layout (_fwd_act, _fwd_neuron), or the refusal."""
        t = l.type
        xb, yb = self.blobs[l.bottoms[0]], self.blobs[l.tops[0]]
        if xb.nchw is None or xb.shape != yb.shape:
            raise NotImplementedError("%s %s on a blob that is neither 4-d nor 2-d" % (t, l.name))
        if xb.esize != yb.esize:
            raise NotImplementedError("f16 engine: %s %s between half and float32 blobs" % (t, l.name))
        grp = 16 // xb.esize
        if xb.coffset % grp or yb.coffset % grp or xb.cstride % grp or yb.cstride % grp:
            raise NotImplementedError("%s %s: a channel window that is not 16-byte aligned" % (t, l.name))
        return xb, yb, xb.pixels, xb.channels

    def _kept_input(self, l: Layer, pix: int, c: int) -> Optional[int]:
        """Pointer of the aux_dev copy (pix x round4(c) floats) that the forward launch of an in-place layer fills with its input - Caffe's
        bottom_memory_ - where this is a TRAIN engine and a gradient comes to the layer; None where nothing is kept."""
        need = getattr(self, "need_grad", None)
        if self.spec.phase != "TRAIN" or l.tops[0] != l.bottoms[0] or not (need is None or l.tops[0] in need):
            return None
        keep = self.aux_dev[l.name] = DeviceBuffer(pix * _r4(c) * 4, zero=True)
        return keep.ptr

    def _fwd_act(self, l: Layer, halves: List[str]) -> List[Op]:
        """PReLU, TanH and Bias as one launch of csrc/act.hip, on whole buffers and on 16-byte-aligned channel windows alike (the kernel
        keeps to its window), floats or halves with float32 parameters.  A TRAIN engine keeps the input of an in-place PReLU to which a
        gradient comes (its bottom needs one, or its slopes learn) in aux_dev, filled by the same launch."""
        lib, t = L.load(), l.type
        xb, yb, pix, c = self._chan_group_views(l)
        mode = L.ACT_MODES[t]
        param = self.params_dev[l.name][0].ptr if t != "TanH" else None
        shared = int(t == "PReLU" and tuple(self.spec.param_shapes[l.name][0]) == ())
        if xb.esize == 2:
            return [Op("act", l.name, lambda st: L.check(lib.fcn_act_fwd_f16(
                xb.buf.ptr, yb.buf.ptr, pix, c, xb.cstride, xb.coffset, yb.cstride, yb.coffset, mode, param, shared, st)), 1.0 * pix * c, 4.0 * pix * c)]
        kp = self._kept_input(l, pix, c) if t == "PReLU" else None
        return [Op("act", l.name, lambda st: L.check(lib.fcn_act_fwd_f32(
            xb.buf.ptr, yb.buf.ptr, kp, pix, c, xb.cstride, xb.coffset, yb.cstride, yb.coffset, _r4(c), mode, param, shared, st)),
            1.0 * pix * c, (8.0 + (4.0 if kp else 0.0)) * pix * c)]

    def _fwd_neuron(self, l: Layer, halves: List[str]) -> List[Op]:
        """ELU, ReLU6, Clip, AbsVal, BNLL and Swish as one launch of csrc/neuron.hip, on whole buffers and on 16-byte-aligned channel
        windows alike (the kernel keeps to its window), floats or halves.  A TRAIN engine keeps the input of an in-place Swish to which a
        gradient comes in aux_dev, filled by the same launch - what _fwd_act does for an in-place PReLU; the other in-place layers read
        their gradient from the top and keep nothing."""
        lib, t = L.load(), l.type
        xb, yb, pix, c = self._chan_group_views(l)
        mode, a, b = neuron_params(l)
        if xb.esize == 2:
            return [Op("neuron", l.name, lambda st: L.check(lib.fcn_neuron_fwd_f16(
                xb.buf.ptr, yb.buf.ptr, pix, c, xb.cstride, xb.coffset, yb.cstride, yb.coffset, mode, a, b, st)), 1.0 * pix * c, 4.0 * pix * c)]
        kp = self._kept_input(l, pix, c) if t == "Swish" else None
        return [Op("neuron", l.name, lambda st: L.check(lib.fcn_neuron_fwd_f32(
            xb.buf.ptr, yb.buf.ptr, kp, pix, c, xb.cstride, xb.coffset, yb.cstride, yb.coffset, _r4(c), mode, a, b, st)),
            1.0 * pix * c, (8.0 + (4.0 if kp else 0.0)) * pix * c)]

    def _fwd_shuffle(self, l: Layer, halves: List[str]) -> List[Op]:
        """ShuffleChannel as one launch of csrc/shuffle.hip, y[j * g + i] = x[i * (C / g) + j] at every pixel, on whole buffers and on
        16-byte-aligned channel windows alike, floats or halves.  The top owns its buffer (storage.plan_blobs never makes it a window of
        the bottom), so the two windows never overlap; nothing is kept for the backward pass."""
        lib = L.load()
        xb, yb, pix, c = self._chan_group_views(l)
        g = shuffle_group(l, [xb.shape])
        if xb.esize == 2:
            return [Op("shuffle", l.name, lambda st: L.check(lib.fcn_shuffle_channel_f16(
                xb.buf.ptr, yb.buf.ptr, pix, c, g, xb.cstride, xb.coffset, yb.cstride, yb.coffset, st)), 0.0, 4.0 * pix * c)]
        return [Op("shuffle", l.name, lambda st: L.check(lib.fcn_shuffle_channel_f32(
            xb.buf.ptr, yb.buf.ptr, pix, c, g, xb.cstride, xb.coffset, yb.cstride, yb.coffset, 0, st)), 0.0, 8.0 * pix * c)]

    def _fwd_dropout(self, l: Layer, halves: List[str]) -> List[Op]:
        lib = L.load()
        xb, yb = self.blobs[l.bottoms[0]], self.blobs[l.tops[0]]
        if self.spec.phase == "TEST":
            return [self._copy_op(l.name, xb, xb.coffset, yb, yb.coffset, xb.pixels, xb.channels)]
        ratio = float(l.sub("dropout_param").get("dropout_ratio", 0.5))
        n, c, h, w = xb.nchw
        salt = dropout_layer_salt(self.spec, l)
        return [Op("dropout", l.name, lambda st: L.check(lib.fcn_dropout_f32(
            xb.buf.ptr, yb.buf.ptr, n, c, h, w, xb.cstride, xb.coffset, yb.cstride, yb.coffset, ratio, (self.dropout_seed + salt) & 0xFFFFFFFF,
            self.dropout_index_offset, st)),
            0.0, 8.0 * xb.pixels * c)]

    def _fwd_loss(self, l: Layer, halves: List[str]) -> List[Op]:
        """L1Loss / EuclideanLoss; in a training engine the same launch writes the gradient of the first bottom."""
        lib = L.load()
        ab, bb, lb = self.blobs[l.bottoms[0]], self.blobs[l.bottoms[1]], self.blobs[l.tops[0]]
        if ab.shape != bb.shape or ab.coffset or bb.coffset or ab.cstride != bb.cstride:
            raise NotImplementedError("loss layer %s on mismatched / sliced blobs" % l.name)
        kind = 0 if l.type == "L1Loss" else 1
        weight = l.loss_weight[0] if l.loss_weight else 1.0
        da = self._loss_grad_ptr(l.bottoms[0])
        self.loss_blobs[l.tops[0]] = float(weight)
        return [Op("loss", l.name, lambda st: L.check(lib.fcn_loss_f32(
            kind, ab.ptr, bb.ptr, da, lb.buf.ptr, ab.pixels, ab.channels, ab.cstride, ab.shape[0], weight, st)),
            0.0, 8.0 * ab.pixels * ab.channels)]

    def _fwd_softmax(self, l: Layer, halves: List[str]) -> List[Op]:
        lib = L.load()
        xb, yb = self.blobs[l.bottoms[0]], self.blobs[l.tops[0]]
        if int(l.sub("softmax_param").get("axis", 1)) != 1 or len(xb.shape) == 3:
            # (an (N, P, C) blob lies as rows of P * C floats: only its last axis, _ssd_tasks, has a kernel - axis 1 would be over P)
            raise NotImplementedError("Softmax over an axis other than channels (layer %s)" % l.name)
        if halves and (xb.esize != 2 or xb.coffset % 8 or yb.coffset % (16 // yb.esize)):
            raise NotImplementedError("f16 engine: Softmax %s from a float32 blob / on an unaligned channel slice" % l.name)
        # the half-float kernel takes one more argument: whether it writes float32 (a net output) or halves
        fn, out_f32 = (lib.fcn_softmax_fwd_f16, (1 if yb.esize == 4 else 0,)) if halves else (lib.fcn_softmax_fwd_f32, ())
        return [Op("softmax", l.name, lambda st: L.check(fn(xb.ptr, yb.ptr, xb.pixels, xb.channels, xb.cstride, yb.cstride, *out_f32, st)),
                   0.0, float(xb.esize + yb.esize) * xb.pixels * xb.channels)]

    def _fwd_softmax_loss(self, l: Layer, halves: List[str]) -> List[Op]:
        lib = L.load()
        xb, lab, lb = self.blobs[l.bottoms[0]], self.blobs[l.bottoms[1]], self.blobs[l.tops[0]]
        if lab.channels != 1 or lab.pixels != xb.pixels or xb.coffset:
            raise NotImplementedError("SoftmaxWithLoss %s: needs one label per pixel of an unsliced score blob" % l.name)
        lp = l.sub("loss_param")
        normalize = 1 if bool(lp.get("normalize", True)) else 0
        ign = lp.get("ignore_label", None)
        weight = l.loss_weight[0] if l.loss_weight else 1.0
        da = self._loss_grad_ptr(l.bottoms[0])
        self.loss_blobs[l.tops[0]] = float(weight)
        ws = DeviceBuffer(int(lib.fcn_softmax_loss_workspace_bytes()), zero=True)
        self._keep.append(ws)
        return [Op("loss", l.name, lambda st: L.check(lib.fcn_softmax_loss_f32(
            xb.ptr, lab.ptr, da, lb.buf.ptr, xb.shape[0], xb.pixels, xb.channels, xb.cstride, lab.cstride, normalize,
            0 if ign is None else 1, 0 if ign is None else int(ign), weight, ws.ptr, st)), 0.0, 8.0 * xb.pixels * xb.channels)]

    def _fwd_accuracy(self, l: Layer, halves: List[str]) -> List[Op]:
        lib, B = L.load(), self.blobs
        if self.f16:
            raise NotImplementedError("f16 engine: layer type Accuracy (%s) has no half-float kernel" % l.name)
        xb, lab, ab = B[l.bottoms[0]], B[l.bottoms[1]], B[l.tops[0]]
        if lab.channels != 1 or lab.pixels != xb.pixels:
            raise NotImplementedError("Accuracy %s: needs one label per pixel of the score blob" % l.name)
        ap = l.sub("accuracy_param")
        if int(ap.get("axis", 1)) != 1:
            raise NotImplementedError("Accuracy over an axis other than channels (layer %s)" % l.name)
        top_k, ign = int(ap.get("top_k", 1)), ap.get("ignore_label", None)
        per_class = B[l.tops[1]].ptr if len(l.tops) > 1 else None
        ws = DeviceBuffer(int(lib.fcn_accuracy_workspace_bytes()), zero=True)
        self._keep.append(ws)
        return [Op("accuracy", l.name, lambda st: L.check(lib.fcn_accuracy_f32(
            xb.ptr, lab.ptr, ab.ptr, per_class, xb.shape[0], xb.pixels, xb.channels, xb.cstride, lab.cstride, top_k,
            0 if ign is None else 1, 0 if ign is None else int(ign), ws.ptr, st)), 0.0, 4.0 * xb.pixels * (xb.channels + 1))]

    def _fwd_slice(self, l: Layer, halves: List[str]) -> List[Op]:
        out, off, xb = [], 0, self.blobs[l.bottoms[0]]
        for tn in l.tops:
            yb = self.blobs[tn]
            out.append(self._copy_op(l.name + ":" + tn, xb, xb.coffset + off, yb, yb.coffset, yb.pixels, yb.channels))
            off += yb.channels
        return out

    def _fwd_concat(self, l: Layer, halves: List[str]) -> List[Op]:
        out, off, yb = [], 0, self.blobs[l.tops[0]]
        for bn in l.bottoms:
            xb = self.blobs[bn]
            out.append(self._copy_op(l.name + ":" + bn, xb, xb.coffset, yb, yb.coffset + off, xb.pixels, xb.channels))
            off += xb.channels
        return out

    def _fwd_eltwise(self, l: Layer, halves: List[str]) -> List[Op]:
        lib, out = L.load(), []
        p = l.sub("eltwise_param")
        opname = str(p.get("operation", "SUM"))
        op = {"PROD": L.ELT_PROD, "SUM": L.ELT_SUM, "MAX": L.ELT_MAX}[opname]
        coeff = [float(c) for c in p.getall("coeff")] or [1.0] * len(l.bottoms)
        yb = self.blobs[l.tops[0]]
        srcs = [self.blobs[b] for b in l.bottoms]
        if halves and len(halves) != len(l.bottoms) + 1:
            raise NotImplementedError("f16 engine: Eltwise %s mixes half and float32 blobs" % l.name)
        for b in srcs + [yb]:
            if not (b.coffset == 0 and b.cstride == yb.cstride):
                raise NotImplementedError("Eltwise on channel slices (layer %s)" % l.name)
        count = yb.pixels * yb.cstride
        fn = lib.fcn_eltwise_fwd_f16 if halves else lib.fcn_eltwise_fwd_f32
        a = srcs[0]
        for i, b in enumerate(srcs[1:], start=1):
            ca = coeff[0] if i == 1 else 1.0
            out.append(Op("eltwise", l.name, lambda st, a=a, b=b, ca=ca, cb=coeff[i]: L.check(fn(
                a.ptr, b.ptr, yb.ptr, count, op, ca, cb, st)), 0.0, 3.0 * yb.esize * count))
            a = yb
        return out

    def _fwd_inner_product(self, l: Layer, relu: bool) -> List[Op]:
        """InnerProduct.  At up to FCN_IP_MAX_ROWS rows: the weight-streaming kernels (csrc/inner_product.hip); above, for a NetSpec
        built with ip_gemm=True: the same call on the matrix-core kernels of csrc/ip_gemm.hip.  The bottom's rows are
        the input vectors as they lie in memory, the bank was packed in that order at upload; the top is N pixels of num_output
        channels, written at its channel offset (a member of a Concat of (N, C) blobs in place: _plan_buffers aliases it)."""
        lib = L.load()
        xb, yb = self.blobs[l.bottoms[0]], self.blobs[l.tops[0]]      # (a whole buffer: storage.param_layout refuses any other bottom)
        m, c, h, w = xb.nchw
        n_out = yb.channels
        k = h * w * xb.cstride
        gemm = m > L.IP_MAX_ROWS
        if gemm and not self.spec.ip_gemm:
            raise NotImplementedError(L.ip_rows_refusal(l.name, m))
        if xb.esize == 4 and yb.esize != 4:
            raise NotImplementedError("f16 engine: InnerProduct %s reads float32 and writes halves" % l.name)
        devs = self.params_dev[l.name]
        bias = devs[1].ptr if len(devs) > 1 else None
        nbytes = int(lib.fcn_ip_gemm_workspace_bytes(m, k, n_out, xb.esize) if gemm else lib.fcn_inner_product_fwd_workspace_bytes(m, k, n_out, xb.esize))
        ws = DeviceBuffer(nbytes, zero=False) if nbytes else None
        if ws is not None:
            self._keep.append(ws)
        wsp = ws.ptr if ws is not None else None
        # non-temporal weight loads: the bank is read once per forward; launched alone behind a 512 MiB memset that policy took
        # 0.5 - 0.9 of the default's time, replayed back to back about the same (not measured inside a net)
        # (the GEMM has no such flag: its tiles of the bank are read again by the workgroups of the other row tiles)
        flags = (L.CONV_RELU if relu else 0) | (0 if gemm else L.IP_WEIGHTS_NT)
        if xb.esize == 2:
            fn, flags = (lib.fcn_ip_gemm_fwd_f16 if gemm else lib.fcn_inner_product_fwd_f16), flags | (L.CONV_OUT_F32 if yb.esize == 4 else 0)
        else:
            fn = lib.fcn_ip_gemm_fwd_f32 if gemm else lib.fcn_inner_product_fwd_f32
        wptr = devs[0].ptr
        return [Op("ip_gemm" if gemm else "inner_product", l.name, lambda st: L.check(fn(xb.buf.ptr, k, wptr, bias, yb.buf.ptr, yb.cstride, yb.coffset, m, k, n_out,
                                                                  flags, wsp, st)),
                   2.0 * m * c * h * w * n_out, float(xb.esize) * (n_out * k + m * k) + float(yb.esize) * m * n_out)]

    def _fwd_deconvolution(self, l: Layer, halves: List[str]) -> List[Op]:
        lib = L.load()
        g = self._geom(l)
        xb, yb = self.blobs[l.bottoms[0]], self.blobs[l.tops[0]]
        c, co, k = g.cin, g.cout, g.k
        wdev = self.params_dev[l.name][0].ptr
        bdev = self.params_dev[l.name][1].ptr if len(self.params_dev[l.name]) > 1 else None
        if self.param_segs[(l.name, 0)].kind == S.DECONV:
            # group 1: the transposed convolution on the matrix cores.  Its bank is re-packed from the blob in front of every
            # launch (one small launch): the blob may have been stepped by a solver, set through net.params or belong to
            # another engine (share_params) since the last forward.
            if self.param_segs[(l.name, 0)].esize == 2:
                return self._fwd_tconv_f16(l, g, xb, yb, wdev, bdev)
            if xb.coffset % 4 or xb.cstride % 4:
                raise NotImplementedError("Deconvolution %s: input view is not 16-byte aligned" % l.name)
            bank = DeviceBuffer(max(int(lib.fcn_tconv_bank_floats(c, co, k, k)), 4) * 4, zero=True)
            d = tconv_desc(xb, yb, g, bank.ptr, bdev)
            tws = DeviceBuffer(int(lib.fcn_tconv2d_workspace_bytes(C.byref(d), 1)), zero=False)
            plan = L.TConvPlan()
            L.call("fcn_tconv2d_prepare", C.byref(d), 1, tws.ptr, -1, C.byref(plan))
            self._keep.extend([bank, d, tws, plan])
            return [Op("tconv_pack", l.name, lambda st: L.check(lib.fcn_tconv_bank_pack_f32(wdev, bank.ptr, c, co, _r4(co), k, k, st)),
                       0.0, 8.0 * c * co * k * k),
                    Op("tconv", l.name, lambda st: L.check(lib.fcn_tconv2d_f32(C.byref(plan), st)),
                       2.0 * g.n * g.h * g.w * c * co * k * k, 4.0 * (xb.pixels * c + yb.pixels * co))]
        if halves and (xb.esize != 2 or xb.coffset % 8):
            raise NotImplementedError("f16 engine: Deconvolution %s from a float32 blob / an unaligned channel slice" % l.name)
        # depthwise (group == channels); the half-float kernel takes one more argument: whether it writes float32 or halves
        fn, out_f32 = (lib.fcn_deconv_depthwise_fwd_f16, (1 if yb.esize == 4 else 0,)) if halves else (lib.fcn_deconv_depthwise_fwd_f32, ())
        return [Op("deconv", l.name, lambda st: L.check(fn(
            xb.ptr, wdev, bdev, yb.buf.ptr, g.n, g.h, g.w, c, xb.cstride, k, g.s, g.pad, g.oh, g.ow, yb.cstride, yb.coffset, *out_f32, st)),
            2.0 * yb.pixels * c * (k / g.s) ** 2, float(xb.esize * xb.pixels + yb.esize * yb.pixels) * c)]

    def _fwd_tconv_f16(self, l: Layer, g: ConvGeom, xb: Blob, yb: Blob, wdev: int, bdev: Optional[int]) -> List[Op]:
        """A group-1 Deconvolution of a half-float engine whose NetSpec was built with tconv_f16=True (storage.param_layout laid its
        blob out in halves): the bottom and the bank hold halves, the bias is float32, the top holds halves or float32 (a net output).
        The bank is re-packed in front of every launch, as in float32."""
        lib = L.load()
        c, co, k = g.cin, g.cout, g.k
        if xb.esize != 2:
            raise NotImplementedError("f16 engine: Deconvolution %s reads the float32 blob %s" % (l.name, l.bottoms[0]))
        if xb.coffset % 8 or xb.cstride % 8:
            raise NotImplementedError("Deconvolution %s: input view is not 16-byte aligned" % l.name)
        bank = DeviceBuffer(max(int(lib.fcn_tconv_bank_halves(c, co, k, k)), 8) * 2, zero=True)
        d = tconv_desc(xb, yb, g, bank.ptr, bdev, L.CONV_OUT_F32 if yb.esize == 4 else 0)
        tws = DeviceBuffer(int(lib.fcn_tconv2d_workspace_bytes(C.byref(d), 1)), zero=False)
        plan = L.TConvPlan()
        L.call("fcn_tconv2d_prepare_f16", C.byref(d), 1, tws.ptr, -1, C.byref(plan))
        self._keep.extend([bank, d, tws, plan])
        return [Op("tconv_pack", l.name, lambda st: L.check(lib.fcn_tconv_bank_pack_f16(wdev, bank.ptr, c, co, _ra(co, 2), k, k, st)),
                   0.0, 4.0 * c * co * k * k),
                Op("tconv", l.name, lambda st: L.check(lib.fcn_tconv2d_f16(C.byref(plan), st)),
                   2.0 * g.n * g.h * g.w * c * co * k * k, 2.0 * xb.pixels * c + float(yb.esize) * yb.pixels * co)]

    # ------------------------------------------------------------------ host <-> device
    def _stage(self, name: str) -> DeviceBuffer:
        st = self._staging.get(name)
        if st is None:
            b = self.blobs[name]
            st = DeviceBuffer(max(int(np.prod(b.shape)) if b.shape else 1, 1) * 4, zero=False)
            self._staging[name] = st
        return st

    def host_array(self, name: str) -> np.ndarray:
        b = self.blobs[name]
        if b.host is None:
            b.pinned = PinnedArray(b.shape)
            b.host = b.pinned.array
        return b.host

    # Host <-> device traffic of a blob is two steps: a COPY between the pinned host array and a device staging buffer (NCHW float32), and
    # a layout KERNEL between the staging buffer and the blob (NHWC, channel stride, element type).  Only the kernels are ever captured
    # into a hipGraph: round 3 held the copies as memcpy nodes of the same graph, and under `rocprofv3 --kernel-trace` hipGraphLaunch of
    # that graph died with SIGSEGV inside the runtime in the process that keeps four replica engines (three of five runs in round 3; once
    # more in round 4 AFTER every kernel of the graph had been launched eagerly before the capture, so a first launch inside the capture
    # was not the cause - profiles/experiments/r04_graph_io_segv_under_rocprofv3.txt).  The graph of kernels alone has never failed, with
    # or without the profiler: the copies are plain hipMemcpyAsync calls on the same stream now, in front of and behind the graph launch.
    def _upload_copy(self, name: str, stream: Optional[int]) -> None:
        b = self.blobs[name]
        host = self.host_array(name)
        dst = b.ptr if b.nchw is None else self._stage(name).ptr
        L.check(L.load().fcn_memcpy_h2d_async(dst, host.ctypes.data, host.nbytes, stream))

    def _upload_convert(self, name: str, stream: Optional[int]) -> None:
        b = self.blobs[name]
        if b.nchw is None:
            return
        lib = L.load()
        n, c, h, w = b.nchw
        st = self._stage(name)
        if b.esize == 2:
            L.check(lib.fcn_nchw_f32_to_nhwc_f16(st.ptr, b.buf.ptr, n, c, h, w, b.cstride, b.coffset, b.upload_shift, stream))
        else:
            L.check(lib.fcn_nchw_to_nhwc_f32(st.ptr, b.buf.ptr, n, c, h, w, b.cstride, b.coffset, b.upload_shift, stream))

    def _download_convert(self, name: str, stream: Optional[int]) -> None:
        b = self.blobs[name]
        if b.nchw is None:
            return
        lib = L.load()
        n, c, h, w = b.nchw
        st = self._stage(name)
        if b.esize == 2:
            L.check(lib.fcn_nhwc_f16_to_nchw_f32(b.buf.ptr, st.ptr, n, c, h, w, b.cstride, b.coffset, stream))
        else:
            L.check(lib.fcn_nhwc_to_nchw_f32(b.buf.ptr, st.ptr, n, c, h, w, b.cstride, b.coffset, stream))

    def _download_convert_all(self, stream: Optional[int]) -> None:
        """The layout kernels of ALL output blobs: the float32 4-d ones share one launch (fcn_nhwc_to_nchw_multi_f32 - behind a batch-1
        forward two launches of a few microseconds each were launch floor, not work), the others take their own."""
        multi = [nm for nm in self.outputs if self.blobs[nm].nchw is not None and self.blobs[nm].esize == 4]
        if 2 <= len(multi) <= 8:
            if not hasattr(self, "_multi_descs"):
                arr = (L.LayoutDesc * len(multi))()
                for d, nm in zip(arr, multi):
                    b = self.blobs[nm]
                    n, c, h, w = b.nchw
                    d.src, d.dst, d.N, d.C, d.H, d.W, d.src_cstride, d.src_coffset = b.buf.ptr, self._stage(nm).ptr, n, c, h, w, b.cstride, b.coffset
                self._multi_descs = arr
            L.check(L.load().fcn_nhwc_to_nchw_multi_f32(self._multi_descs, len(multi), stream))
        else:
            multi = []
        for nm in self.outputs:
            if nm not in multi:
                self._download_convert(nm, stream)

    def _download_copy(self, name: str, stream: Optional[int]) -> None:
        b = self.blobs[name]
        host = self.host_array(name)
        src = b.ptr if b.nchw is None else self._stage(name).ptr
        L.check(L.load().fcn_memcpy_d2h_async(host.ctypes.data, src, host.nbytes, stream))

    def _enqueue_upload(self, name: str, stream: Optional[int]) -> None:
        self._upload_copy(name, stream)
        self._upload_convert(name, stream)

    def _enqueue_download(self, name: str, stream: Optional[int]) -> None:
        self._download_convert(name, stream)
        self._download_copy(name, stream)

    def read_blob(self, name: str) -> np.ndarray:
        """Synchronised NCHW float32 host copy of a blob (pycaffe ``net.blobs[name].data``)."""
        if name in self.spec.mask_blobs:
            return self._read_mask(name)
        if name in self.rpn_views:     # a middle blob of the RPN softmax chain: its neighbour's NCHW array in Caffe's memory order
            return np.ascontiguousarray(self.read_blob(self.rpn_views[name])).reshape(self.shapes[name])
        if name in self.permutes:      # Caffe's (N, H, W, C) array, read from the bottom's buffer
            return np.ascontiguousarray(self.read_blob(self.permutes[name]).transpose(0, 2, 3, 1))
        if name in self.spec.prior_blobs:
            return self.prior_consts[name]
        if name in self.detections:
            with self.lock:
                L.call("fcn_init", self.device)
                b = self.blobs[name]
                self.host_array(name)
                if not b.host_valid:
                    self._enqueue_download(name, self.stream)
                    L.call("fcn_stream_sync", self.stream)
                    b.host_valid = True
                return self._compose_detections(name)
        with self.lock:
            L.call("fcn_init", self.device)
            b = self.blobs[name]
            host = self.host_array(name)
            if not b.host_valid:
                for op in self._lazy_blob_ops.get(name, ()):      # a blob a fused launch skipped: its own layer, on demand
                    op.run(self.stream)
                self._enqueue_download(name, self.stream)
                L.call("fcn_stream_sync", self.stream)
                if b.lazy_shift:
                    host += F32(b.lazy_shift)
                b.host_valid = True
            return self._cut_rois(name, host)

    def _read_mask(self, name: str) -> np.ndarray:
        """A pooling mask as Caffe holds it: NCHW float32, the flat iy * W + ix index of each window's maximum in the plane of the
        pooling's bottom.  The device keeps the pooling's int32 argmax buffer; this converts a copy (fcn_pool_mask_to_nchw_f32)."""
        with self.lock:
            L.call("fcn_init", self.device)
            n, c, ph, pw = self.shapes[name]
            idx = self.aux_dev[self.spec.mask_blobs[name].name]
            host = np.empty((n, c, ph, pw), F32)
            tmp = DeviceBuffer(host.nbytes, zero=False)
            try:
                L.call("fcn_pool_mask_to_nchw_f32", idx.ptr, tmp.ptr, n, ph, pw, c, self.stream)
                L.call("fcn_memcpy_d2h_async", host.ctypes.data, tmp.ptr, host.nbytes, self.stream)
                L.call("fcn_stream_sync", self.stream)
            finally:
                tmp.free()
            return host

    # ------------------------------------------------------------------ label grids generated on the device
    # blob names of the DetectNet label tops, in the order DataArgumentationLayer emits them (data_argumentation_layer.py:67-72)
    LABEL_TOPS = ("coverage-label", "bbox-label", "size-block", "obj-block", "coverage-block")

    def set_targets(self, rects: Sequence[Sequence[Sequence[int]]], labels: Sequence[Sequence[int]], stride: int,
                    iou_thresh: float = 0.1, tops: Sequence[str] = LABEL_TOPS) -> None:
        """Stage the ground-truth boxes of the next step; the label blobs are then generated ON THE DEVICE inside step() / forward_score()
        (fcn_gen_targets_nhwc: bounding_box_parameterized_labels of the reference) instead of being uploaded."""
        fg = self.blobs[tops[0]]
        n, c, gy, gx = fg.shape
        if len(rects) != n or len(labels) != n:
            raise ValueError("need boxes for %d images" % n)
        offs = np.zeros(n + 1, np.int32)
        flat_r, flat_l = [], []
        for i, (rs, ls) in enumerate(zip(rects, labels)):
            for r, lab in zip(rs, ls):
                if not 0 <= int(lab) < c:
                    raise IndexError("label %d outside [0, %d)" % (lab, c))
                flat_r.append([int(v) for v in r])
                flat_l.append(int(lab))
            offs[i + 1] = len(flat_r)
        if not hasattr(self, "_tgt"):
            cap = max(64 * n, 256)
            self._tgt = dict(cap=cap, rects=DeviceBuffer(cap * 16, zero=True), labels=DeviceBuffer(cap * 4, zero=True),
                             offs=DeviceBuffer((n + 1) * 4, zero=True))
        if len(flat_r) > self._tgt["cap"]:
            raise ValueError("too many boxes in one batch (%d > %d)" % (len(flat_r), self._tgt["cap"]))
        self._tgt.update(h_rects=np.asarray(flat_r, np.int32).reshape(-1, 4), h_labels=np.asarray(flat_l, np.int32), h_offs=offs,
                         stride=int(stride), thresh=float(iou_thresh), tops=tuple(tops), pending=True)

    def _enqueue_targets(self) -> None:
        t, lib = self._tgt, L.load()
        if t["h_rects"].size:
            L.check(lib.fcn_memcpy_h2d_async(t["rects"].ptr, t["h_rects"].ctypes.data, t["h_rects"].nbytes, self.stream))
            L.check(lib.fcn_memcpy_h2d_async(t["labels"].ptr, t["h_labels"].ctypes.data, t["h_labels"].nbytes, self.stream))
        L.check(lib.fcn_memcpy_h2d_async(t["offs"].ptr, t["h_offs"].ctypes.data, t["h_offs"].nbytes, self.stream))
        fg, bb, sz, ob, cv = (self.blobs[nm] for nm in t["tops"])
        n, c, gy, gx = fg.shape
        for b in (bb, sz, ob, cv):
            if b.coffset or b.cstride != bb.cstride:
                raise NotImplementedError("label blobs must be plain buffers of one geometry")
        L.check(lib.fcn_gen_targets_nhwc(t["rects"].ptr, t["labels"].ptr, t["offs"].ptr, n, c, gy, gx, t["stride"], t["thresh"],
                                         fg.ptr, fg.cstride, bb.ptr, sz.ptr, ob.ptr, cv.ptr, bb.cstride, self.stream))


    # ------------------------------------------------------------------ scoring (Solver::Test, `caffe test`)
    def score_begin(self, io: bool = False) -> None:
        """Start of a test pass: zero every accumulator (one fcn_memset_async each) on the engine's stream.  The forward graph is
        captured first: its warm-up launches would otherwise land in the accumulators.  io=True: the pass will run through
        forward() (outputs downloaded per batch, what `caffe test` prints) instead of forward_score()."""
        if not self.score_outputs:
            raise RuntimeError("engine was not built with score_outputs=True")
        with self.lock:
            L.call("fcn_init", self.device)
            for nm in self.inputs:
                if nm not in self.device_fed:
                    self.host_array(nm)
                    if self.blobs[nm].nchw is not None:
                        self._stage(nm)
            if graphs_enabled():
                if io and self.graph_io is None:
                    for nm in self.outputs:
                        self.host_array(nm)
                    self.graph_io = self._capture(with_io=True)
                elif not io and self.graph_score is None:
                    self.graph_score = self._capture(with_io=True, download=False)
            for acc in self.score_acc.values():
                L.call("fcn_memset_async", acc.ptr, 0, acc.nbytes, self.stream)
            self.score_forwards = 0

    def forward_score(self, uploaded_event=None) -> None:
        """One forward of a test pass, enqueued without waiting: copies of the host-fed inputs, staged label grids, then ONE graph launch
        (layout kernels of the inputs, every layer, the accumulation of every output blob).  Nothing is read back.  uploaded_event is
        recorded behind the input copies: the host arrays may be refilled once it has passed."""
        with self.lock:
            for nm in self.inputs:      # (label tops generated by set_targets() belong in device_fed, like rendered scenes)
                if nm not in self.device_fed:
                    self._upload_copy(nm, self.stream)
            if uploaded_event is not None:
                L.call("fcn_event_record", uploaded_event, self.stream)
            if getattr(self, "_tgt", None) is not None and self._tgt.get("pending"):
                self._enqueue_targets()
            if self.graph_score is not None:
                L.call("fcn_graph_launch", self.graph_score, self.stream)
            else:
                for nm in self.inputs:
                    if nm not in self.device_fed:
                        self._upload_convert(nm, self.stream)
                self.run_ops(self.stream)
            for b in self.blobs.values():
                b.host_valid = False
            self.score_forwards += 1

    def score_read(self) -> Dict[str, np.ndarray]:
        """End of a test pass: the one read-back.  {output blob: float32 sums over the forwards since score_begin(), blob shape}."""
        with self.lock:
            out = {nm: np.empty(self.blobs[nm].shape, F32) for nm in self.outputs}
            for nm, a in out.items():
                L.call("fcn_memcpy_d2h_async", a.ctypes.data, self.score_acc[nm].ptr, a.nbytes, self.stream)
            L.call("fcn_stream_sync", self.stream)
            return out

    # ------------------------------------------------------------------ execution
    def run_ops(self, stream: Optional[int]) -> None:
        for op in self.ops:
            op.run(stream)

    def _capture(self, with_io: bool, download: bool = True) -> int:
        if with_io:                      # nothing may allocate while the stream is capturing
            for nm in list(self.inputs) + list(self.outputs):
                self.host_array(nm)
                if self.blobs[nm].nchw is not None:
                    self._stage(nm)
        if not getattr(self, "_warm", False):
            # code objects load lazily on a kernel's first launch, which must not happen inside a stream capture
            self.run_ops(self.stream)
            L.call("fcn_stream_sync", self.stream)
            self._warm = True
        if with_io and not getattr(self, "_warm_io", False):
            # the same for the layout kernels of the upload and - never launched by anything else before the first forward() - of the
            # download: one eager pass (the host arrays end up holding the outputs of the warm pass)
            for nm in self.inputs:
                if nm not in self.device_fed:
                    self._enqueue_upload(nm, self.stream)
            self._download_convert_all(self.stream)
            for nm in self.outputs:
                self._download_copy(nm, self.stream)
            L.call("fcn_stream_sync", self.stream)
            self._warm_io = True
        L.call("fcn_graph_begin", self.stream)
        try:
            if with_io:      # layout kernels only: the copies stay outside the graph (see _upload_copy)
                for nm in self.inputs:
                    if nm not in self.device_fed:
                        self._upload_convert(nm, self.stream)
            self.run_ops(self.stream)
            if with_io and download:
                self._download_convert_all(self.stream)
        finally:
            g = C.c_void_p()
            L.call("fcn_graph_end", self.stream, C.byref(g))
        return int(g.value)

    def _launch_io(self) -> None:
        """Copies in, the graph of layout kernels + layers, copies out - all on the engine's stream, nothing waits."""
        if self.graph_io is None:
            self.graph_io = self._capture(with_io=True)
        for nm in self.inputs:
            if nm not in self.device_fed:
                self._upload_copy(nm, self.stream)
        L.call("fcn_graph_launch", self.graph_io, self.stream)
        for nm in self.outputs:
            self._download_copy(nm, self.stream)
        self._download_counts(self.stream)

    def forward(self, use_graph: bool = True) -> Dict[str, np.ndarray]:
        """Upload inputs, run every layer, download the output blobs (synchronous, like Net.forward())."""
        use_graph = use_graph and graphs_enabled()
        with self.lock:
            L.call("fcn_init", self.device)
            for nm in self.inputs:
                self.host_array(nm)
            for nm in self.outputs:
                self.host_array(nm)
            if use_graph:
                self._launch_io()
            else:
                for nm in self.inputs:
                    if nm not in self.device_fed:
                        self._enqueue_upload(nm, self.stream)
                self.run_ops(self.stream)
                for nm in self.outputs:
                    self._enqueue_download(nm, self.stream)
                self._download_counts(self.stream)
            L.call("fcn_stream_sync", self.stream)
            for b in self.blobs.values():
                b.host_valid = False
            self._ran = self._counts_valid = True      # (the Proposal counts came down behind the layers)
            out = {}
            for nm in self.outputs:
                b = self.blobs[nm]
                if b.lazy_shift:
                    b.host += F32(b.lazy_shift)
                b.host_valid = True
                out[nm] = self._cut_rois(nm, b.host) if nm not in self.detections else self._compose_detections(nm)
            for nm in self.inputs:
                self.blobs[nm].host_valid = nm not in self.device_fed
            return out

    def forward_begin(self) -> None:
        """Enqueue upload + layers + download of one forward and return without waiting (forward_end() collects)."""
        with self.lock:
            L.call("fcn_init", self.device)
            for nm in list(self.inputs) + list(self.outputs):
                self.host_array(nm)
            if graphs_enabled():
                self._launch_io()
            else:
                for nm in self.inputs:
                    if nm not in self.device_fed:
                        self._enqueue_upload(nm, self.stream)
                self.run_ops(self.stream)
                for nm in self.outputs:
                    self._enqueue_download(nm, self.stream)
                self._download_counts(self.stream)

    def forward_end(self) -> Dict[str, np.ndarray]:
        with self.lock:
            L.call("fcn_stream_sync", self.stream)
            for b in self.blobs.values():
                b.host_valid = False
            self._ran = self._counts_valid = True      # (the Proposal counts came down behind the layers)
            out = {}
            for nm in self.outputs:
                b = self.blobs[nm]
                if b.lazy_shift:
                    b.host += F32(b.lazy_shift)
                b.host_valid = True
                out[nm] = self._cut_rois(nm, b.host) if nm not in self.detections else self._compose_detections(nm)
            for nm in self.inputs:
                self.blobs[nm].host_valid = nm not in self.device_fed
            return out

    def upload_inputs(self) -> None:
        with self.lock:
            for nm in self.inputs:
                self._enqueue_upload(nm, self.stream)
            L.call("fcn_stream_sync", self.stream)

    def forward_enqueue(self) -> None:
        """The layer stack once on inputs already in HBM, enqueued on the engine's stream without waiting."""
        with self.lock:
            if graphs_enabled():
                if self.graph_core is None:
                    self.graph_core = self._capture(with_io=False)
                L.call("fcn_graph_launch", self.graph_core, self.stream)
            else:
                self.run_ops(self.stream)
            for b in self.blobs.values():
                if not b.is_input:
                    b.host_valid = False
            self._ran, self._counts_valid = True, False

    def forward_resident(self, iters: int = 1, use_graph: bool = True) -> float:
        """Run the layer stack ``iters`` times on inputs already in HBM; returns HIP-event ms for all iterations."""
        use_graph = use_graph and graphs_enabled()      # plain launches (e.g. under a profiler)
        with self.lock:
            L.call("fcn_init", self.device)
            if use_graph and self.graph_core is None:
                self.graph_core = self._capture(with_io=False)
            e0, e1 = C.c_void_p(), C.c_void_p()
            L.call("fcn_event_create", C.byref(e0))
            L.call("fcn_event_create", C.byref(e1))
            L.call("fcn_event_record", e0, self.stream)
            for _ in range(iters):
                if use_graph:
                    L.call("fcn_graph_launch", self.graph_core, self.stream)
                else:
                    self.run_ops(self.stream)
            L.call("fcn_event_record", e1, self.stream)
            L.call("fcn_event_sync", e1)
            ms = C.c_float()
            L.call("fcn_event_elapsed_ms", e0, e1, C.byref(ms))
            L.call("fcn_event_destroy", e0)
            L.call("fcn_event_destroy", e1)
            for b in self.blobs.values():
                if not b.is_input:
                    b.host_valid = False
            self._counts_valid = False
            return float(ms.value)

    def time_ops(self, reps: int = 20, ops: Optional[Sequence["Op"]] = None) -> List[Tuple[str, str, float, float, float]]:
        """Per-op HIP-event timing (ms) on the engine's stream: [(kind, name, ms, flops, bytes)]."""
        out = []
        with self.lock:
            e0, e1 = C.c_void_p(), C.c_void_p()
            L.call("fcn_event_create", C.byref(e0))
            L.call("fcn_event_create", C.byref(e1))
            for op in (self.ops if ops is None else ops):
                op.run(self.stream)
                L.call("fcn_event_record", e0, self.stream)
                for _ in range(reps):
                    op.run(self.stream)
                L.call("fcn_event_record", e1, self.stream)
                L.call("fcn_event_sync", e1)
                ms = C.c_float()
                L.call("fcn_event_elapsed_ms", e0, e1, C.byref(ms))
                out.append((op.kind, op.name, ms.value / reps, op.flops, op.bytes))
            L.call("fcn_event_destroy", e0)
            L.call("fcn_event_destroy", e1)
        return out

    def time_ops_in_sequence(self, reps: int = 10) -> List[Tuple[str, str, float, float, float]]:
        """Per-op HIP-event timing (ms) with every launch in the cache state it has inside a forward pass: for op i the ops
        0 .. i-1 run (untimed) in front of it, then event, op i, event.  time_ops() repeats ONE launch back to back, so its
        operands (the filters above all) come from a warm L2 - in a real forward the 24 MB of filters and the activations of the
        other 26 launches have passed through the 4 MB L2s in between; rocprofv3's per-kernel durations of a forward are the
        in-sequence ones and are matched by this method.  (The reading of an EMPTY event pair, ~2 us, is kept in
        `event_pair_floor_ms` but NOT subtracted: the second event's processing overlaps the kernel's completion - with it
        subtracted the family came out 16 % faster than rocprofv3's own durations, without it the two agree.)"""
        out = []
        with self.lock:
            e0, e1 = C.c_void_p(), C.c_void_p()
            L.call("fcn_event_create", C.byref(e0))
            L.call("fcn_event_create", C.byref(e1))
            ms = C.c_float()
            empty = []
            for _ in range(10):      # what two events with nothing between them read
                self.ops[0].run(self.stream)
                L.call("fcn_event_record", e0, self.stream)
                L.call("fcn_event_record", e1, self.stream)
                L.call("fcn_event_sync", e1)
                L.call("fcn_event_elapsed_ms", e0, e1, C.byref(ms))
                empty.append(ms.value)
            floor = float(np.median(empty))
            for i, op in enumerate(self.ops):
                acc = []
                for _ in range(reps):
                    for prev in self.ops[:i]:
                        prev.run(self.stream)
                    L.call("fcn_event_record", e0, self.stream)
                    op.run(self.stream)
                    L.call("fcn_event_record", e1, self.stream)
                    L.call("fcn_event_sync", e1)
                    L.call("fcn_event_elapsed_ms", e0, e1, C.byref(ms))
                    acc.append(ms.value)
                out.append((op.kind, op.name, float(np.median(acc)), op.flops, op.bytes))
            L.call("fcn_event_destroy", e0)
            L.call("fcn_event_destroy", e1)
        self.event_pair_floor_ms = floor
        return out

    def close(self) -> None:
        with self.lock:
            lib = L.load()
            for g in (self.graph_io, self.graph_core, self.graph_score):
                if g:
                    lib.fcn_graph_destroy(g)
            self.graph_io = self.graph_core = self.graph_score = None
            if self.stream:
                lib.fcn_stream_sync(self.stream)
                lib.fcn_stream_destroy(self.stream)
                self.stream = 0
            # the library's host copies of this engine's prepared groups are keyed by their workspace address: drop them before
            # the addresses can be handed out again
            for ws in self._group_workspaces:
                if ws.ptr:
                    lib.fcn_conv2d_group_release(ws.ptr)
                    ws.free()
            self._group_workspaces = []
            self.ops = []
            self.tuner.release()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class ForwardPipeline:
    """Several frames in flight on one GPU.

    A batch-1 forward of the DetectNet stack is 27 launches of 5-40 us that each fill the chip for only part of their
    duration (one round of <= 600 workgroups, then a tail): a single stream leaves the MI355X half idle.  The pipeline keeps
    `depth` replicas of the engine - own stream, own activation arena, same weights and the first replica's tile plan - and
    hands consecutive frames to them round-robin, so the hardware queues interleave the launches of different frames
    How many workgroups of DIFFERENT launches fit on a CU is bounded by LDS, so the replicas' autotuner is restricted to tile
    configurations of at most `max_lds_kb` per workgroup: this costs nothing on a lone stream (2530 frames/s either way) and
    is worth +20 % once frames overlap.  Each replica takes a replica stream (fcn_stream_create_replica): a hardware queue of its
    own also under the runtime's default limit of four queues.  Measured, kernels only: about 3600 frames/s one frame at a time,
    4840-4900 with three in flight, 5400-5440 with four at either queue limit (round 3, plain streams and 16 queues: 2530 /
    4000-4130 / 4300-4480, and 3400 with five - a fifth replica takes a plain stream and has not been measured since).  Per-frame results are those of a lone engine
    with the same tile plan, bit for bit: the replicas run the same kernels on private buffers."""

    def __init__(self, make_spec: Callable[[], NetSpec], params: Optional[Dict[str, List[np.ndarray]]] = None, device: int = 0, depth: int = 4,
                 max_lds_kb: Optional[int] = 36, **engine_kw):
        if depth < 1:
            raise ValueError("depth must be at least 1")
        self.engines: List[Engine] = []
        if os.environ.get("FCN_PIPE_LDS_KB"):      # (experiments: another cap, 0 = none)
            max_lds_kb = int(os.environ["FCN_PIPE_LDS_KB"]) or None
        if max_lds_kb is not None:
            engine_kw.setdefault("tune_max_lds_kb", max_lds_kb)
        for i in range(depth):
            self.engines.append(Engine(make_spec(), params=params, device=device, tune_from=self.engines[0] if i else None, replica=i,
                                       **engine_kw))
        self._pending: List[Engine] = []
        self._next = 0

    @property
    def depth(self) -> int:
        return len(self.engines)

    def submit(self, inputs: Dict[str, np.ndarray]) -> None:
        """Start the forward of one frame; at most `depth` frames may be outstanding (collect() frees a slot)."""
        if len(self._pending) >= len(self.engines):
            raise RuntimeError("ForwardPipeline: %d frames already in flight, collect() one first" % len(self._pending))
        eng = self.engines[self._next]
        self._next = (self._next + 1) % len(self.engines)
        for nm, arr in inputs.items():
            eng.host_array(nm)[...] = arr
        eng.forward_begin()
        self._pending.append(eng)

    def collect(self) -> Dict[str, np.ndarray]:
        """Outputs of the OLDEST outstanding frame (copies: the replica's host arrays are reused by later frames)."""
        if not self._pending:
            raise RuntimeError("ForwardPipeline: nothing in flight")
        eng = self._pending.pop(0)
        return {k: v.copy() for k, v in eng.forward_end().items()}

    def map(self, frames: Sequence[Dict[str, np.ndarray]]) -> List[Dict[str, np.ndarray]]:
        """Forward of every frame, `depth` at a time, results in input order."""
        out: List[Dict[str, np.ndarray]] = []
        for f in frames:
            if len(self._pending) == len(self.engines):
                out.append(self.collect())
            self.submit(f)
        while self._pending:
            out.append(self.collect())
        return out

    def calibrate(self, depths: Sequence[int] = (3, 4), iters: int = 60) -> int:
        """Pick how many replicas run_resident() uses: how launches of different streams pack onto the hardware queues is
        not monotonic in the number of streams, so the candidates are timed once (untimed warm-up work for a benchmark)."""
        best, best_t = None, 1e30
        for d in depths:
            if 1 <= d <= len(self.engines):
                self.run_resident(iters, depth=d)
                t = self.run_resident(iters, depth=d)
                if t < best_t:
                    best, best_t = d, t
        self.active = best or len(self.engines)
        return self.active

    def run_resident(self, iters: int, depth: Optional[int] = None) -> float:
        """`iters` forwards in total, round-robin over the first `depth` replicas (default: calibrate()'s choice, else all),
        on inputs already in HBM; wall-clock seconds from the first launch to the last replica draining (benchmarks)."""
        import time
        lib = L.load()
        engines = self.engines[:depth or getattr(self, "active", None) or len(self.engines)]
        return self._run_resident(engines, iters, lib, time)

    def run_io(self, iters: int, depth: Optional[int] = None) -> float:
        """`iters` forwards INCLUDING the transfers (SURVEY 8(d) config 2's region: H2D of the input blob from the replica's pinned
        host array, layout change, all kernels, D2H of the outputs into pinned host arrays), `depth` frames in flight: a frame's
        copies ride on its replica's stream, so they overlap the kernels of the other replicas.  Wall-clock seconds."""
        import time
        engines = self.engines[:depth or getattr(self, "active", None) or len(self.engines)]
        pending: List[Engine] = []
        t0 = time.perf_counter()
        for i in range(iters):
            e = engines[i % len(engines)]
            if len(pending) == len(engines):
                pending.pop(0).forward_end()
            e.forward_begin()
            pending.append(e)
        while pending:
            pending.pop(0).forward_end()
        return time.perf_counter() - t0

    def warm_io(self, depth: Optional[int] = None) -> None:
        """One untimed forward with transfers per replica: captures each replica's graph with the copy nodes (benchmarks call it before run_io)."""
        for e in self.engines[:depth or getattr(self, "active", None) or len(self.engines)]:
            e.forward_begin()
            e.forward_end()

    def _run_resident(self, engines, iters, lib, time) -> float:
        for e in engines:
            if e.graph_core is None:
                e.forward_resident(1)
            L.call("fcn_stream_sync", e.stream)
        no_graph = not graphs_enabled()
        t0 = time.perf_counter()
        for i in range(iters):
            e = engines[i % len(engines)]
            if no_graph:
                e.run_ops(e.stream)
            else:
                L.check(lib.fcn_graph_launch(e.graph_core, e.stream))
        for e in engines:
            L.call("fcn_stream_sync", e.stream)
        return time.perf_counter() - t0

    def close(self) -> None:
        for e in self.engines:
            e.close()
