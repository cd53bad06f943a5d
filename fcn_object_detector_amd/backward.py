"""Plan of the backward pass of a TrainEngine: layer list in reverse -> the launches of Net::Backward.

Runs once, when the engine is built.  One method per layer type (BackwardPlanner.emitters / .one_bottom); what they share is the
write state of every gradient view - state() / mark() - because a gradient that already holds a value must be accumulated
into, and because the LAST data-gradient pass that writes a view may take the ReLU mask of the layer below into its epilogue
(_finish_dgrads).
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Dict, List, Optional, Tuple

from . import lib as L
from . import storage as S
from .engine import Blob, DevView, DeviceBuffer, Op, _r4, conv_desc, dropout_layer_salt, dwconv_desc, rconv_desc, tconv_desc
from .netspec import (DATA_TYPES, NEURON_TYPES, SHUFFLE_TYPES, Layer, crop_window, interp_size, is_rectangular, is_scale_gate, kernel_stride_pad, layer_dilation,
                      neuron_params, scale_gate_form, shuffle_group)


@dataclass
class Dgrad:
    """One data-gradient launch, prepared once the whole plan is known: a group of stride-1 passes that write different buffers
    (ConvDesc, launch: L.ConvGroup), the transposed convolution of one strided layer (TConvDesc, launch: L.TConvPlan), the
    convolution of dY with the flipped bank of one dilated or rectangular layer (RConvDesc, launch: L.RConvPlan), or the gather of one
    depthwise layer (DwConvDesc, launch: None - nothing to prepare).
    targets[i]: the blob descs[i] writes.  shows: what the op's label shows of the geometry once the launch is prepared."""
    name: str
    descs: list
    targets: List[str]
    launch: object
    op: Optional[Op] = None
    shows: str = ""


# the plan class of a one-problem data-gradient launch -> prefix of its entry points
_SINGLE_DGRAD = {L.RConvPlan: "fcn_rconv2d", L.TConvPlan: "fcn_tconv2d"}


@dataclass
class PoolBwd:
    """A MAX pooling backward writing the gradient of `blob`; mask = (activation buffer, cstride, coffset) once the ReLU backward
    of that blob is folded into it."""
    blob: str
    mask: Tuple[Optional[int], int, int] = (None, 0, 0)


class BackwardPlanner:
    def __init__(self, eng) -> None:
        self.e, self.spec, self.B, self.G, self.lib = eng, eng.spec, eng.blobs, eng.grad_blobs, L.load()
        self.ops: List[Op] = []
        self.ws_floats = 1                                   # workspace of the weight-gradient launches: the largest any of them needs
        self.ip_ws_bytes = 0                                 # ... and of the InnerProduct data gradients, which run beside them (_inner_product)
        self.ip_wgrad_ws_bytes = 0                           # ... and of the InnerProduct weight gradients above FCN_IP_MAX_ROWS rows (csrc/ip_gemm.hip)
        self.gate_ws_bytes = 0                               # ... and of the gate gradients of the gated Scale layers (csrc/gate.hip)
        self.act_ws_bytes = 0                                # ... and of the parameter gradients of PReLU and Bias layers (csrc/act.hip)
        self.written: Dict[int, List[Tuple[int, int]]] = {}  # gradient buffer -> channel ranges already holding a gradient
        self.writers: Dict[str, List[object]] = {}           # gradient blob -> what wrote it, in order (a dgrad / pooling record or None)
        self.concat_members: Dict[str, List[str]] = {}       # Concat output -> its member blobs
        self.concat_relu: Dict[str, str] = {}                # member blob -> the Concat output one ReLU mask launch covers
        self.relu_done, self.dgrad_done, self.wgrad_done = set(), set(), set()
        self.sibling_reduces: Dict[str, List[Layer]] = {}    # reduce layer -> the reduce layers of its module (ready together)
        self.flip_layout: Dict[str, int] = {}                # stride-1 convolution -> offset of its bank in flip_flat (floats)
        self.flip_segs_dev: Optional[DeviceBuffer] = None
        self.tbank: Dict[str, DeviceBuffer] = {}
        self.dgrad_records: List[Dgrad] = []
        self.relu_ops: Dict[str, Op] = {}                    # gradient blob whose ReLU backward is the op (candidates for the fused mask)
        self.skip_sigmoid_of = {m["sigmoid_top"]: name for name, m in eng._conv_layer_meta.items() if m.get("sigmoid_top")}
        nothing = lambda l: None
        # layer types that look at the plan state themselves ...
        self.emitters = {"Convolution": self._convolution, "DepthwiseConvolution": self._convolution, "InnerProduct": self._inner_product, "Eltwise": self._eltwise, "Deconvolution": self._deconvolution,
                         "Sigmoid": self._sigmoid, "ReLU": self._relu, "Slice": self._slice, "Concat": self._concat,
                         "BatchNorm": self._batchnorm, "Scale": lambda l: (self._scale_gate if is_scale_gate(l) else self._batchnorm)(l),
                         "L1Loss": self._loss, "EuclideanLoss": self._loss, "SoftmaxWithLoss": self._loss,
                         "Accuracy": nothing,      # a metric: no gradient, no entry in loss_blobs
                         **{t: nothing for t in DATA_TYPES}}
        # ... and the ones _one_bottom hands (layer, dY, dX, accumulate)
        self.one_bottom = {"Pooling": self._pooling, "LRN": self._lrn, "Dropout": self._dropout, "Eltwise": self._eltwise_prod,
                           "Deconvolution": self._depthwise_deconv, "Sigmoid": self._sigmoid_plain, "ReLU": self._relu_plain,
                           "Crop": self._crop, "Interp": self._interp, "Upsample": self._upsample,
                           "Power": lambda l, gtop, gbot, acc: None}      # input transform: nothing upstream learns
        # ... and the one-bottom activations of csrc/act.hip, which _one_bottom consults where one_bottom has no entry: the same
        # (layer, dY, dX, accumulate), except that dX is None where only the layer's own blob wants a gradient
        self.activations = {"PReLU": self._act, "TanH": self._act, "Bias": self._act}
        # ... and those of csrc/neuron.hip (no learned blob), which _one_bottom consults after the two tables above
        self.neurons = {t: self._neuron for t in NEURON_TYPES}
        # ... and the channel shuffle of csrc/shuffle.hip, a fifth table that _one_bottom consults last
        self.shuffles = {t: self._shuffle for t in SHUFFLE_TYPES}

    def run(self) -> None:
        self._find_concat_relu()
        self._plan_banks()
        for l in reversed(self.spec.layers):
            (self.emitters.get(l.type) or self._one_bottom)(l)
        self._finish_dgrads()
        self.ws = DeviceBuffer(self.ws_floats * 4, zero=False)
        self.ip_ws = DeviceBuffer(self.ip_ws_bytes, zero=False) if self.ip_ws_bytes else None
        self.ip_wgrad_ws = DeviceBuffer(self.ip_wgrad_ws_bytes, zero=False) if self.ip_wgrad_ws_bytes else None
        self.gate_ws = DeviceBuffer(self.gate_ws_bytes, zero=False) if self.gate_ws_bytes else None
        self.act_ws = DeviceBuffer(self.act_ws_bytes, zero=False) if self.act_ws_bytes else None

    # ------------------------------------------------------------------ write state of the gradient views
    def state(self, g: Blob) -> str:
        """'none' | 'full' for the channel range of view g (partial overlap is a planning error)."""
        lo, hi = g.coffset, g.coffset + g.channels
        cov = 0
        for a, b in self.written.get(g.buf.ptr, []):
            o = min(hi, b) - max(lo, a)
            if o > 0:
                cov += o
        if cov == 0:
            return "none"
        if cov >= hi - lo:
            return "full"
        raise NotImplementedError("gradient of %s is partially written" % g.name)

    def mark(self, g: Blob, writer: object = None) -> None:
        self.written.setdefault(g.buf.ptr, []).append((g.coffset, g.coffset + g.channels))
        self.writers.setdefault(g.name, []).append(writer)

    def last_writer(self, name: str) -> object:
        w = self.writers.get(name)
        return w[-1] if w else None

    def _arrived(self, l: Layer) -> Optional[Blob]:
        """dY of the layer's first top, or None when no gradient reaches this layer."""
        g = self.G.get(l.tops[0]) if l.tops else None
        return g if g is not None and self.state(g) != "none" else None

    # ------------------------------------------------------------------ before the layers
    def _conv_of(self, blob: str) -> Layer:
        return [q for q in self.e.producers.get(blob, []) if q.type == "Convolution"][0]

    def _rconv(self, l: Layer) -> bool:
        """A Convolution that csrc/rconv.hip runs (engine._rconv_task): rectangular, or square with dilation > 1."""
        return l.type == "Convolution" and not self.spec.is_depthwise(l) and (layer_dilation(l) > 1 or is_rectangular(l))

    def _own_kernel(self, l: Layer) -> bool:
        """A Convolution that csrc/rconv.hip or csrc/dwconv.hip runs (engine._rconv_task, engine._dwconv_task): it stays out of the
        grouped dense launches."""
        return self.spec.is_depthwise(l) or self._rconv(l)

    def _find_concat_relu(self) -> None:
        """Concat outputs all of whose members are convolutions with a fused in-place ReLU: their ReLU backward is one launch."""
        e, B = self.e, self.B
        for child, (parent, _off) in e.alias.items():
            if any(q.type == "Concat" and parent in q.tops for q in e.producers.get(parent, [])):
                self.concat_members.setdefault(parent, []).append(child)
        for parent, members in self.concat_members.items():
            prods = [[q for q in e.producers.get(m, []) if q.type == "Convolution"] for m in members]
            if all(len(pr) == 1 and e._conv_layer_meta.get(pr[0].name, {}).get("relu") and not self._own_kernel(pr[0]) for pr in prods) and \
                    sum(B[m].channels for m in members) == B[parent].channels and B[parent].coffset == 0:
                for m in members:
                    self.concat_relu[m] = parent

    def _plan_banks(self) -> None:
        """Filter banks of the data-gradient passes, refreshed from the current weights at the start of every backward pass.
        Stride 1: flipped / transposed banks, slices of ONE flat buffer that a single launch refreshes (58 launches otherwise).
        Strided convolutions: the transposed-convolution kernel reads the layer's own OHWI bank re-packed tap-major
        ([kh][kw][Cin][Cout4])."""
        e, lib = self.e, self.lib
        flip_segs: List[L.FlipSeg] = []
        flip_floats = 0
        packs: List[Op] = []
        for l in self.spec.layers:
            if l.type != "Convolution" or self.G.get(l.bottoms[0]) is None or self.G.get(l.tops[0]) is None:
                continue
            if self.spec.is_depthwise(l):      # the data gradient gathers through the layer's own bank: nothing to flip or pack
                continue
            if self._rconv(l):      # the data gradient is the same kernel on the flipped bank: strides 1, pad' = d (k-1) - pad >= 0 per axis
                r = e._rgeom(l)
                rect = is_rectangular(l)      # (a square layer is named as a dilated one, with one stride and one pad)
                kind = "rectangular" if rect else "dilated"
                axes = (("_h", r.ph, r.kh), ("_w", r.pw, r.kw)) if rect else (("", r.ph, r.kh),)
                if r.sh != 1 or r.sw != 1:
                    raise NotImplementedError("%s Convolution %s: the data gradient of a %s layer with stride %s (its bottom %s needs a gradient)"
                                              % (kind, l.name, kind, "%dx%d" % (r.sh, r.sw) if rect else r.sh, l.bottoms[0]))
                for axis, pad, k in axes:
                    if pad > r.d * (k - 1):
                        raise NotImplementedError("%s Convolution %s: the data gradient with pad%s %d above dilation * (kernel%s - 1) = %d (its "
                                                  "bottom %s needs a gradient)" % (kind, l.name, axis, pad, axis, r.d * (k - 1), l.bottoms[0]))
                self.flip_layout[l.name] = flip_floats
                wdev = e.params_dev[l.name][0].ptr
                flip_segs.append(L.FlipSeg((wdev - e.param_flat.ptr) // 4, flip_floats, r.cout, r.kh, r.kw, r.cin, _r4(r.cin), _r4(r.cout)))
                flip_floats += _r4(r.cin * r.kh * r.kw * _r4(r.cout))
                continue
            g, ng = e._geom(l), e._conv_groups(l)
            cin, cout, k = g.cin // ng, g.cout // ng, g.k      # of one group: its bank is rows i*cout .. of the layer's (storage.conv_groups)
            if g.s == 1:
                self.flip_layout[l.name] = flip_floats
            for i in range(ng):
                wdev = e.params_dev[l.name][0].ptr + 4 * i * cout * k * k * _r4(cin)
                if g.s == 1:
                    flip_segs.append(L.FlipSeg((wdev - e.param_flat.ptr) // 4, flip_floats, cout, k, k, cin, _r4(cin), _r4(cout)))
                    flip_floats += self._flip_floats(cin, cout, k)
                else:
                    bank = self.tbank[self._tbank_key(l, i)] = DeviceBuffer(max(int(lib.fcn_tconv_bank_floats(cout, cin, k, k)), 4) * 4, zero=True)
                    packs.append(Op("tconv_pack", self._tbank_key(l, i), lambda st, wdev=wdev, bank=bank, cout=cout, cin=cin, k=k: L.check(
                        lib.fcn_tconv_bank_pack_f32(wdev, bank.ptr, cout, cin, _r4(cin), k, k, st))))
        self.flip_flat = DeviceBuffer(max(flip_floats, 4) * 4, zero=True)
        if flip_segs:
            seg_arr = (L.FlipSeg * len(flip_segs))(*flip_segs)
            self.flip_segs_dev = DeviceBuffer(C.sizeof(seg_arr), zero=False)
            L.call("fcn_memcpy_h2d_async", self.flip_segs_dev.ptr, C.addressof(seg_arr), C.sizeof(seg_arr), None)
            L.call("fcn_device_sync")
            self.ops.append(Op("flip", "%d filter banks" % len(flip_segs), lambda st, n=len(flip_segs): L.check(lib.fcn_conv_weights_flip_batch_f32(
                e.param_flat.ptr, e._flip_flat.ptr, e._flip_segs_dev.ptr, n, st))))
        self.ops.extend(packs)

    @staticmethod
    def _flip_floats(cin: int, cout: int, k: int) -> int:
        """Floats of one flipped bank [cin][k][k][r4(cout)] in flip_flat."""
        return _r4(cin * k * k * _r4(cout))

    @staticmethod
    def _tbank_key(l: Layer, group: int) -> str:
        return l.name if group == 0 else "%s#%d" % (l.name, group)

    # ------------------------------------------------------------------ data gradients
    def emit_tdgrad(self, l: Layer, gtop: Blob, gbot: Blob, accumulate: bool, group: int = 0) -> Dgrad:
        """Data gradient of the strided convolution l: the transposed convolution of dY, written at the size of the layer's input
        (rows / columns of it that lay under no window get zeros).  Prepared in _finish_dgrads like the grouped launches, because
        the ReLU mask of the layer below may still be folded into its epilogue."""
        g, lib, ng = self.e._geom(l), self.lib, self.e._conv_groups(l)
        if gtop.coffset % 4 or gtop.cstride - gtop.coffset < _r4(g.cout):
            raise NotImplementedError("gradient view of %s is not a 16-byte aligned run of whole channel groups" % l.tops[0])
        if g.pad >= g.k:
            raise NotImplementedError("data gradient of the strided convolution %s with pad %d >= kernel %d" % (l.name, g.pad, g.k))
        cin_g, cout_g = g.cin // ng, g.cout // ng
        d = tconv_desc(gtop, gbot, g.swapped()._replace(cin=cout_g, cout=cin_g), self.tbank[self._tbank_key(l, group)].ptr,
                       flags=L.CONV_ACCUM if accumulate else 0)
        d.a += 4 * group * cout_g           # the group's channels of dY ...
        d.b_coffset += group * cin_g        # ... make its channels of dX
        rec = Dgrad(self._tbank_key(l, group), [d], [l.bottoms[0]], L.TConvPlan())
        rec.op = Op("tconv_dgrad", rec.name, lambda st, pl=rec.launch: L.check(lib.fcn_tconv2d_f32(C.byref(pl), st)), g.flops / (ng * ng))
        self.ops.append(rec.op)
        self.dgrad_records.append(rec)
        self.e._keep.append(d)
        return rec

    def dgrad_desc(self, l: Layer, gtop: Blob, gbot: Blob, accumulate: bool, group: int = 0) -> Tuple[L.ConvDesc, float]:
        """Data gradient of convolution l (of its group `group`) = the forward kernel on dY with the flipped / transposed bank: a group
        reads its Cout/g channels of dY and writes its Cin/g channels of dX."""
        g, ng = self.e._geom(l), self.e._conv_groups(l)
        if g.s != 1:
            raise RuntimeError("dgrad_desc is the stride-1 path; strided layers go through emit_tdgrad (%s)" % l.name)
        cin_g, cout_g = g.cin // ng, g.cout // ng
        cin_dg = _r4(cout_g)      # the flipped bank reads Cout4 input channels: the gradient view must expose them contiguously
        if gtop.cstride - gtop.coffset - group * cout_g < cin_dg:
            raise NotImplementedError("gradient view of %s too narrow for the data-gradient pass" % l.tops[0])
        wt = DevView(self.flip_flat.ptr + 4 * (self.flip_layout[l.name] + group * self._flip_floats(cin_g, cout_g, g.k)), cin_g * g.k * g.k * cin_dg * 4)
        dd = conv_desc(gtop, gbot, g.swapped()._replace(cin=cin_dg, cout=cin_g, s=1, pad=g.k - 1 - g.pad), wt.ptr,
                       flags=L.CONV_ACCUM if accumulate else 0)
        dd.x += 4 * group * cout_g
        dd.y_coffset += group * cin_g
        self.e._keep.append(dd)
        return dd, g.flops / (ng * ng)

    def emit_dgrads(self, name: str, items: List[Tuple[L.ConvDesc, float]], targets: List[str]) -> Dgrad:
        """One grouped launch for data-gradient passes that write different buffers.  The group is prepared (and
        autotuned) after the whole backward plan is known, because the LAST writer of a gradient may still get the ReLU
        mask of the layer below folded into its epilogue (_finish_dgrads)."""
        lib = self.lib
        rec = Dgrad(name, [d for d, _ in items], list(targets), L.ConvGroup())
        rec.op = Op("dgrad", name, lambda st, g=rec.launch: L.check(lib.fcn_conv2d_fwd_group_f32(C.byref(g), st)), sum(fl for _, fl in items))
        self.ops.append(rec.op)
        self.dgrad_records.append(rec)
        return rec

    def _finish_dgrads(self) -> None:
        e, B, lib = self.e, self.B, self.lib
        # fold "ReLU backward of blob X" into the last data-gradient pass that writes dX, when that is what wrote it last
        for x, rop in self.relu_ops.items():
            rec = self.last_writer(x)
            if rec is None or rop not in self.ops:
                continue
            if isinstance(rec, PoolBwd):        # the last writer is a pooling backward of exactly this blob
                if rec.blob == x:
                    rec.mask = (B[x].buf.ptr, B[x].cstride, B[x].coffset)
                    self.ops.remove(rop)
                continue
            act = B[x]
            if x not in rec.targets:
                raise RuntimeError("the last writer of the gradient of %s does not name it among its targets" % x)
            for d, t in zip(rec.descs, rec.targets):      # (the groups of a grouped convolution each write their own channels of dX)
                if t == x:
                    # (a depthwise pass writes the whole view of dX through d.x: its mask starts where the activation's view does)
                    first = d.b_coffset if isinstance(d, L.TConvDesc) else self.G[x].coffset if isinstance(d, L.DwConvDesc) else d.y_coffset
                    d.y2, d.y2_cstride, d.y2_coffset = act.buf.ptr, act.cstride, act.coffset + first - self.G[x].coffset
                    d.flags |= L.CONV_MASK
            self.ops.remove(rop)
        for rec in self.dgrad_records:
            if rec.launch is None:      # a depthwise gather: one pure launch on its descriptor
                continue
            prefix = _SINGLE_DGRAD.get(type(rec.launch))
            if prefix is not None:
                d = rec.descs[0]
                ws = DeviceBuffer(int(getattr(lib, prefix + "_workspace_bytes")(C.byref(d), 1)), zero=False)
                L.call(prefix + "_prepare", C.byref(d), 1, ws.ptr, -1, C.byref(rec.launch))
                e._keep.extend([ws, rec.launch])
                rec.op.name = "%s [%s%dwg]" % (rec.name, rec.shows, rec.launch.total_tiles)
                continue
            n_ = len(rec.descs)
            arr = (L.ConvDesc * n_)(*rec.descs)
            gws = DeviceBuffer(int(lib.fcn_conv2d_group_workspace_bytes(n_)), zero=False)
            cfg = e.tuner.conv_cfg("dgrad:" + rec.name, arr, n_, gws) if e.autotune else -1
            L.call("fcn_conv2d_group_prepare", arr, n_, gws.ptr, cfg, C.byref(rec.launch))
            e._keep.extend([arr, gws, rec.launch])
            e._group_workspaces.append(gws)
            rec.op.name = "%s [cfg%d %dwg]" % (rec.name, rec.launch.cfg, rec.launch.total_tiles)

    # ------------------------------------------------------------------ weight gradients, ReLU masks
    def relu_bwd_op(self, name: str, y: Blob, dy: Blob) -> Op:
        """dY = dY where the activation y is positive, else 0, in place: the mask of a ReLU fused into its convolution (slope 0 always:
        engine._relu_after fuses no other; a ReLU layer of its own goes through _relu_plain)."""
        lib = self.lib
        op = Op("relu_bwd", name, lambda st: L.check(lib.fcn_relu_bwd_f32(dy.ptr, y.ptr, dy.ptr, y.pixels, y.channels, y.cstride, st)), 0.0,
                12.0 * y.pixels * y.channels)
        self.ops.append(op)
        return op

    def _book_wgrad(self, op: Op, sel: Optional[dict], names: List[str], ws_floats: List[int]) -> None:
        """A weight-gradient launch: kind "wgrad" puts it on the step's second stream, op.layers tells the data-parallel exchange which
        buckets wait for it, op.sel (None: one form only) is what Tuner.wgrad_cfgs() chooses."""
        self.ws_floats = max([self.ws_floats] + ws_floats)
        op.sel = sel
        op.layers = names
        self.ops.append(op)
        self.wgrad_done.update(names)

    def _wgrad_cfgs(self) -> List[int]:
        return [-1] + (list(range(int(self.lib.fcn_conv2d_wgrad_num_configs()))) if self.e.autotune else [])

    def wgrad_op(self, name: str, d: L.ConvDesc, dw: DevView, db: Optional[DevView], flops: float) -> None:
        """The weight (and bias) gradient of one problem: d.x the layer's input, d.y its dY."""
        e, lib = self.e, self.lib
        sel = {"cfg": -1}      # -1: the library's heuristic; Tuner.wgrad_cfgs() replaces it once the workspace exists
        op = Op("wgrad", name, lambda st: L.check(lib.fcn_conv2d_wgrad_cfg_f32(
            C.byref(d), dw.ptr, db.ptr if db else None, e._ws.ptr, sel["cfg"], st)), flops)
        self._book_wgrad(op, sel, [name], [int(lib.fcn_conv2d_wgrad_workspace_floats_cfg(C.byref(d), c, None)) for c in self._wgrad_cfgs()])

    def wgrad_items(self, l: Layer, gtop: Blob) -> List[Tuple[L.ConvDesc, DevView, Optional[DevView], float]]:
        """(descriptor with y = dY of the layer, dW view, db view or None, flops) of a layer that learns: one per group, dW and db at
        the group's rows."""
        if self._own_kernel(l):
            raise RuntimeError("wgrad_items is the dense path; dilated and rectangular layers have emitters of their own (%s)" % l.name)
        e, g, xb, ng = self.e, self.e._geom(l), self.B[l.bottoms[0]], self.e._conv_groups(l)
        if gtop.coffset % 4 or gtop.cstride % 4:
            raise NotImplementedError("gradient view of %s is not 16-byte aligned" % l.tops[0])
        cin_g, cout_g = g.cin // ng, g.cout // ng
        dw = e._grad_view(l.name, 0)
        db = e._grad_view(l.name, 1) if len(e.params_dev[l.name]) > 1 else None
        out = []
        for i in range(ng):
            d = conv_desc(xb, gtop, g._replace(cin=_r4(cin_g), cout=cout_g))
            d.x += 4 * i * cin_g
            d.y_coffset += i * cout_g
            e._keep.append(d)
            rows = cout_g * g.k * g.k * _r4(cin_g)
            out.append((d, DevView(dw.ptr + 4 * i * rows, 4 * rows), DevView(db.ptr + 4 * i * cout_g, 4 * cout_g) if db is not None else None,
                        g.flops / (ng * ng)))
        return out

    def emit_wgrads(self, layers_: List[Layer], gtops: List[Blob]) -> None:
        """Weight (and bias) gradients of layers that are ready together: one launch + one reduction for up to four."""
        e, lib = self.e, self.lib
        todo = [(l_.name, it) for l_, g_ in zip(layers_, gtops) if e._learns(l_) and l_.name not in self.wgrad_done
                for it in self.wgrad_items(l_, g_)]
        for base in range(0, len(todo), 4):
            chunk = todo[base:base + 4]
            its = [it for _, it in chunk]
            names = list(dict.fromkeys(nm for nm, _ in chunk))      # (the groups of a grouped layer are items of one name)
            if len(its) == 1:
                self.wgrad_op(names[0], *its[0])
                continue
            descs, dws, dbs, flops = zip(*its)
            m = len(its)
            sel = {"cfg": -1}
            arr = (L.ConvDesc * m)(*descs)
            pdw = (C.c_void_p * m)(*[dw.ptr for dw in dws])
            pdb = (C.c_void_p * m)(*[(db.ptr if db is not None else None) for db in dbs])
            e._keep.extend([arr, pdw, pdb])
            op = Op("wgrad", "+".join(names), lambda st, arr=arr, pdw=pdw, pdb=pdb, m=m, sel=sel: L.check(
                lib.fcn_conv2d_wgrad_group_cfg_f32(arr, pdw, pdb, m, e._ws.ptr, sel["cfg"], st)), sum(flops))
            self._book_wgrad(op, sel, names, [int(lib.fcn_conv2d_wgrad_group_workspace_floats_cfg(arr, m, c)) for c in self._wgrad_cfgs()])

    # ------------------------------------------------------------------ Convolution
    def _own_relu_mask(self, l: Layer, gtop: Blob) -> None:
        """The layer's own fused ReLU mask on dY, once per top; the op is remembered (for _finish_dgrads to fold into the data gradient
        of the layer above) unless the top is an alias."""
        top = l.tops[0]
        if self.e._conv_layer_meta[l.name].get("relu") and top not in self.relu_done:
            rop = self.relu_bwd_op(l.name, self.B[top], gtop)
            if top not in self.e.alias:
                self.relu_ops[top] = rop
            self.relu_done.add(top)

    def _rconv_convolution(self, l: Layer, gtop: Blob) -> None:
        """Backward of a dilated or rectangular Convolution (csrc/rconv.hip): the layer's own ReLU mask on dY, the weight gradient on
        the second stream (one form only: op.sel is None), and dX = the same convolution of dY with the flipped bank, strides 1,
        pad_h' = d (kh-1) - pad_h, pad_w' = d (kw-1) - pad_w, accumulating where dX already holds a gradient; _finish_dgrads may fold
        the ReLU mask of the layer below into it, as for a dense pass.  The op of a square layer is a "dconv_dgrad" whose label shows
        the dilation, that of a rectangular one an "rconv_dgrad" that shows the kernel."""
        e, G, lib, top = self.e, self.G, self.lib, l.tops[0]
        g, xb = e._rgeom(l), self.B[l.bottoms[0]]
        self._own_relu_mask(l, gtop)
        if e._learns(l) and l.name not in self.wgrad_done:
            d = rconv_desc(xb, gtop, g)
            dw = e._grad_view(l.name, 0)
            db = e._grad_view(l.name, 1).ptr if len(e.params_dev[l.name]) > 1 else None
            e._keep.append(d)
            op = Op("wgrad", l.name, lambda st: L.check(lib.fcn_rconv2d_wgrad_f32(C.byref(d), dw.ptr, db, e._ws.ptr, st)), g.flops, g.bytes)
            # (the launch runs on the second stream behind the other weight gradients, never beside them: it shares their workspace)
            self._book_wgrad(op, None, [l.name], [int(lib.fcn_rconv2d_wgrad_workspace_floats(C.byref(d)))])
        gbot = G.get(l.bottoms[0])
        if gbot is None or l.name in self.dgrad_done:
            return
        if gtop.coffset % 4 or gtop.cstride % 4 or gtop.cstride - gtop.coffset < _r4(g.cout):
            raise NotImplementedError("gradient view of %s is not a 16-byte aligned run of whole channel groups" % top)
        wt = self.flip_flat.ptr + 4 * self.flip_layout[l.name]
        dd = rconv_desc(gtop, gbot, g.swapped()._replace(sh=1, sw=1, ph=g.d * (g.kh - 1) - g.ph, pw=g.d * (g.kw - 1) - g.pw), wt,
                        flags=L.CONV_ACCUM if self.state(gbot) == "full" else 0)
        rect = is_rectangular(l)
        rec = Dgrad(l.name, [dd], [l.bottoms[0]], L.RConvPlan(), shows="%dx%d " % (g.kh, g.kw) if rect else "d%d " % g.d)
        rec.op = Op("rconv_dgrad" if rect else "dconv_dgrad", rec.name, lambda st, pl=rec.launch: L.check(lib.fcn_rconv2d_f32(C.byref(pl), st)), g.flops)
        self.ops.append(rec.op)
        self.dgrad_records.append(rec)
        e._keep.append(dd)
        self.mark(gbot, rec)

    def _depthwise_convolution(self, l: Layer, gtop: Blob) -> None:
        """Backward of a depthwise Convolution (csrc/dwconv.hip), the shape of _rconv_convolution: the layer's own ReLU mask on dY, the
        weight gradient on the second stream in the shared workspace (one form only: op.sel is None), and dX = the gather of dY through
        the layer's own bank - any stride, no flipped bank - accumulating where dX already holds a gradient; _finish_dgrads may fold the
        ReLU mask of the layer below into it, as for a dense pass."""
        e, G, lib = self.e, self.G, self.lib
        g, xb = e._dwgeom(l), self.B[l.bottoms[0]]
        self._own_relu_mask(l, gtop)
        if e._learns(l) and l.name not in self.wgrad_done:
            d = dwconv_desc(xb, gtop, g)
            dw = e._grad_view(l.name, 0)
            db = e._grad_view(l.name, 1).ptr if len(e.params_dev[l.name]) > 1 else None
            e._keep.append(d)
            op = Op("wgrad", l.name, lambda st: L.check(lib.fcn_dwconv2d_wgrad_f32(C.byref(d), dw.ptr, db, e._ws.ptr, 0, st)), g.flops, g.bytes)
            # (the launch runs on the second stream behind the other weight gradients, never beside them: it shares their workspace)
            self._book_wgrad(op, None, [l.name], [int(lib.fcn_dwconv2d_wgrad_workspace_floats(C.byref(d), 0))])
        gbot = G.get(l.bottoms[0])
        if gbot is None or l.name in self.dgrad_done:
            return
        if gbot.coffset % 4 or gbot.cstride % 4:
            raise NotImplementedError("depthwise Convolution %s: the gradient view of %s is not 16-byte aligned" % (l.name, l.bottoms[0]))
        dd = dwconv_desc(gbot, gtop, g, e.params_dev[l.name][0].ptr, flags=L.CONV_ACCUM if self.state(gbot) == "full" else 0)
        rec = Dgrad(l.name, [dd], [l.bottoms[0]], None)
        rec.op = Op("dwconv_dgrad", "%s [%dx%d]" % (l.name, g.kh, g.kw), lambda st: L.check(lib.fcn_dwconv2d_dgrad_f32(C.byref(dd), -1, st)), g.flops, g.bytes)
        self.ops.append(rec.op)
        self.dgrad_records.append(rec)
        e._keep.append(dd)
        self.mark(gbot, rec)

    def _convolution(self, l: Layer) -> None:
        gtop = self._arrived(l)
        if gtop is None:
            return
        if self.spec.is_depthwise(l):
            return self._depthwise_convolution(l, gtop)
        if self._rconv(l):
            return self._rconv_convolution(l, gtop)
        e, G, top = self.e, self.G, l.tops[0]
        if e._conv_layer_meta[l.name].get("relu") and top not in self.relu_done:
            whole = self.concat_relu.get(top)
            if whole is not None and whole in G and self.state(G[whole]) == "full":
                self._concat_module(whole)
            else:
                self._own_relu_mask(l, gtop)
        self._sibling_wgrads(l)
        self.emit_wgrads([l], [gtop])
        gbot = G.get(l.bottoms[0])
        if gbot is not None and l.name not in self.dgrad_done:
            acc, ng = self.state(gbot) == "full", e._conv_groups(l)
            if e._geom(l).s != 1:
                recs = [self.emit_tdgrad(l, gtop, gbot, acc, i) for i in range(ng)]
                rec = recs[0] if ng == 1 else None      # (no single launch writes all of dX: the ReLU mask below stays a launch of its own)
            else:
                rec = self.emit_dgrads(l.name, [self.dgrad_desc(l, gtop, gbot, acc, i) for i in range(ng)], [l.bottoms[0]] * ng)
            self.mark(gbot, rec)

    def _concat_module(self, whole: str) -> None:
        """Every member of this Concat is a convolution with an in-place ReLU and the gradient of the whole concatenation is
        final: ONE contiguous launch masks all members (an inception module: 4 -> 1); then their data gradients, their weight
        gradients, and which of the layers below become ready together."""
        members = self.concat_members[whole]
        self.relu_ops[whole] = self.relu_bwd_op(whole, self.B[whole], self.G[whole])
        self.relu_done.update(members)
        self._member_dgrads(members)
        # ... and their weight gradients need nothing else either: one grouped launch
        mem_layers = [self._conv_of(m) for m in members]
        self.emit_wgrads(mem_layers, [self.G[m] for m in members])
        self._find_sibling_reduces(mem_layers)

    def _member_dgrads(self, members: List[str]) -> None:
        """The members' data gradients only need the masked gradient of the concatenation and write four different buffers (the
        module input and the outputs of the reduce / pool layers): one grouped launch at the top of the module's backward
        instead of four scattered ones."""
        G = self.G
        items, names, targets, tnames = [], [], [], []
        for m in members:
            lm = self._conv_of(m)
            gb = G.get(lm.bottoms[0])
            if gb is None or lm.name not in self.flip_layout or self.state(gb) != "none" or any(gb.buf.ptr == tb for tb in targets) \
                    or self.e._conv_groups(lm) != 1:
                continue
            items.append(self.dgrad_desc(lm, G[m], gb, False))
            names.append(lm.name)
            targets.append(gb.buf.ptr)
            tnames.append(lm.bottoms[0])
        if len(items) > 1:
            rec = self.emit_dgrads("+".join(names), items, tnames)
            for nm, tn in zip(names, tnames):
                self.dgrad_done.add(nm)
                self.mark(G[tn], rec)

    def _find_sibling_reduces(self, mem_layers: List[Layer]) -> None:
        """The layers feeding the members (3x3_reduce, 5x5_reduce) get their whole gradient from the members' dgrad launch: they
        become ready together too."""
        e = self.e
        sibs = []
        for lm in mem_layers:
            if lm.name not in self.dgrad_done:
                continue
            prods = [q for q in e.producers.get(lm.bottoms[0], []) if q.type == "Convolution"]
            cons = [q for q in e.consumers.get(lm.bottoms[0], []) if not (q.type in ("ReLU", "Dropout") and q.bottoms == q.tops)]
            if len(prods) == 1 and len(cons) == 1 and lm.bottoms[0] not in e.alias and lm.bottoms[0] in self.G and not self._own_kernel(prods[0]):
                sibs.append(prods[0])
        if len(sibs) > 1:
            for q in sibs:
                self.sibling_reduces[q.name] = sibs

    def _sibling_wgrads(self, l: Layer) -> None:
        """l is the first of its module's reduce layers to be visited: mask and take the weight gradients of all of them now."""
        G = self.G
        sibs = self.sibling_reduces.get(l.name)
        if not (sibs and l.name not in self.wgrad_done and all(self.state(G[q.tops[0]]) == "full" for q in sibs)):
            return
        for q in sibs:
            if q.tops[0] not in self.relu_done and self.e._conv_layer_meta[q.name].get("relu"):
                self.relu_ops[q.tops[0]] = self.relu_bwd_op(q.name, self.B[q.tops[0]], G[q.tops[0]])
                self.relu_done.add(q.tops[0])
        self.emit_wgrads(sibs, [G[q.tops[0]] for q in sibs])

    # ------------------------------------------------------------------ InnerProduct
    def _inner_product(self, l: Layer) -> None:
        """The weight-streaming kernels of csrc/inner_product.hip at M <= FCN_IP_MAX_ROWS rows, the matrix-core kernels of
        csrc/ip_gemm.hip above (NetSpec ip_gemm=True; the same operands, op kinds ip_gemm_bwd / wgrad): dW / db from the layer's input
        rows and dY, dX = dY x bank.  Rows of the bottom and of its gradient are H*W*cstride floats apart and the bank holds zeros in the columns
        of the pad channels, so pad channels of dX and pad columns of dW come out zero: the solver, weight decay and clipping run over
        the packed buffer as it is."""
        gtop = self._arrived(l)
        if gtop is None:
            return
        e, lib, top = self.e, self.lib, l.tops[0]
        xb = self.B[l.bottoms[0]]
        m, c, h, w = xb.nchw
        k, n_out = h * w * xb.cstride, gtop.channels
        gemm = m > L.IP_MAX_ROWS
        if gemm and not self.spec.ip_gemm:
            raise NotImplementedError(L.ip_rows_refusal(l.name, m))
        gemm_ws = int(lib.fcn_ip_gemm_workspace_bytes(m, k, n_out, 4)) if gemm else 0
        if e._conv_layer_meta[l.name].get("relu") and top not in self.relu_done:
            self.relu_bwd_op(l.name, self.B[top], gtop)      # the layer's own in-place ReLU, on dY first
            self.relu_done.add(top)
        if e._learns(l) and l.name not in self.wgrad_done:
            dw = e._grad_view(l.name, 0)
            db = e._grad_view(l.name, 1).ptr if len(e.params_dev[l.name]) > 1 else None
            if gemm:
                # a workspace of the weight gradients' own (for all such layers: they run one after the other on the second stream, beside
                # bwd_data and its slabs)
                self.ip_wgrad_ws_bytes = max(self.ip_wgrad_ws_bytes, gemm_ws)
                op = Op("wgrad", l.name, lambda st: L.check(lib.fcn_ip_gemm_bwd_weights_f32(
                    xb.buf.ptr, k, gtop.buf.ptr, gtop.cstride, gtop.coffset, dw.ptr, db, m, k, n_out, 0,
                    e._ip_wgrad_ws.ptr if e._ip_wgrad_ws is not None else None, st)),
                    2.0 * m * c * h * w * n_out, 4.0 * (n_out * k + m * k + m * n_out))
            else:
                op = Op("wgrad", l.name, lambda st: L.check(lib.fcn_inner_product_bwd_weights_f32(
                    xb.buf.ptr, k, gtop.buf.ptr, gtop.cstride, gtop.coffset, dw.ptr, db, m, k, n_out, 0, st)),
                    2.0 * m * c * h * w * n_out, 4.0 * (n_out * k + m * k + m * n_out))
            self._book_wgrad(op, None, [l.name], [])
        gbot = self.G.get(l.bottoms[0])
        if gbot is None:
            return
        if gbot.coffset or gbot.cstride != xb.cstride or gbot.cstride != _r4(c):      # (storage.param_layout refused the forward's already)
            raise NotImplementedError("InnerProduct %s: the gradient of the bottom %s is a channel window of a wider buffer" % (l.name, l.bottoms[0]))
        # the slabs of bwd_data are NOT the weight gradients' workspace: those launches run on the second stream at the same time
        self.ip_ws_bytes = max(self.ip_ws_bytes, gemm_ws if gemm else int(lib.fcn_inner_product_workspace_bytes(m, k, n_out)))
        flags = L.CONV_ACCUM if self.state(gbot) == "full" else 0
        wptr = e.params_dev[l.name][0].ptr
        fn = lib.fcn_ip_gemm_bwd_data_f32 if gemm else lib.fcn_inner_product_bwd_data_f32
        self.ops.append(Op("ip_gemm_bwd" if gemm else "inner_product_bwd", l.name, lambda st: L.check(fn(
            gtop.buf.ptr, gtop.cstride, gtop.coffset, wptr, gbot.buf.ptr, k, m, k, n_out, flags,
            e._ip_ws.ptr if e._ip_ws is not None else None, st)),
            2.0 * m * c * h * w * n_out, 4.0 * (n_out * k + m * k + m * n_out)))
        self.mark(gbot)

    # ------------------------------------------------------------------ the other layers that look at the plan state themselves
    def _slice(self, l: Layer) -> None:
        if l.name in self.e.copy_slices and any(tp in self.G for tp in l.tops):
            raise NotImplementedError("backward through the copied Slice %s" % l.name)

    def _concat(self, l: Layer) -> None:
        """A Concat whose members are views of its top has nothing to do: their gradients are views of its gradient.  One that copies
        (a member with other consumers, or written by a layer that cannot write a channel window) hands every member its channels of dY:
        the Crop adjoint over the whole extent, adding where the member's gradient already holds one."""
        if l.name not in self.e.copy_concats:
            return
        gtop = self._arrived(l)
        if gtop is None:
            return
        lib, off = self.lib, 0
        for b in l.bottoms:
            gbot, c = self.G.get(b), self.B[b].channels
            if gbot is not None:
                acc = 1 if self.state(gbot) == "full" else 0
                n, _, h, w = gbot.nchw
                self.ops.append(Op("concat_bwd", "%s:%s" % (l.name, b), lambda st, gbot=gbot, c=c, off=off, acc=acc, n=n, h=h, w=w: L.check(lib.fcn_crop_bwd_f32(
                    gtop.buf.ptr, gbot.buf.ptr, n, h, w, c, gbot.cstride, gbot.coffset, 0, 0, h, w, gtop.cstride, gtop.coffset + off, acc, st)),
                    0.0, 4.0 * gbot.pixels * c * (2 + acc)))
                self.mark(gbot)
            off += c

    def _loss(self, l: Layer) -> None:
        g = self.G.get(l.bottoms[0])
        if g is None:
            return
        if l.bottoms[1] in self.e.need_grad:
            raise NotImplementedError("loss layer %s: gradient w.r.t. the second bottom" % l.name)
        if self.state(g) != "none":
            raise NotImplementedError("loss gradient would have to accumulate into %s (%s)" % (l.bottoms[0], l.name))
        self.mark(g)                      # written by the forward loss kernel (da)

    def _sigmoid(self, l: Layer) -> None:
        if l.tops[0] not in self.skip_sigmoid_of:
            return self._one_bottom(l)
        # fused into the conv epilogue in forward; backward is its own small kernel
        yb, gtop, gbot = self.B[l.tops[0]], self.G.get(l.tops[0]), self.G.get(l.bottoms[0])
        if gtop is None or gbot is None or self.state(gtop) == "none":
            return
        lib, acc = self.lib, 1 if self.state(gbot) == "full" else 0
        count = yb.pixels * yb.cstride
        if yb.coffset or gtop.coffset or gbot.coffset or yb.cstride != gbot.cstride:
            raise NotImplementedError("sigmoid backward on channel slices (%s)" % l.name)
        self.ops.append(Op("sigmoid_bwd", l.name, lambda st: L.check(lib.fcn_sigmoid_bwd_f32(yb.ptr, gtop.ptr, gbot.ptr, count, acc, st))))
        self.mark(gbot)

    def _relu(self, l: Layer) -> None:
        if l.name not in self.e._fused_relu_layers():
            self._one_bottom(l)

    def _eltwise(self, l: Layer) -> None:
        p = l.sub("eltwise_param")
        if str(p.get("operation", "SUM")) != "SUM":
            return self._one_bottom(l)
        gtop = self._arrived(l)
        if gtop is None:
            return
        # d(bottom_i) = dY for every bottom (train/fcn_bbox fuse_pool4 / fuse_pool3: skip connections)
        if any(float(c) != 1.0 for c in p.getall("coeff")):
            raise NotImplementedError("Eltwise SUM backward with coefficients (%s)" % l.name)
        lib = self.lib
        for bn in l.bottoms:
            gb = self.G.get(bn)
            if gb is None:
                continue
            if self.state(gb) == "full":
                if gtop.coffset or gb.coffset or gb.cstride != gtop.cstride:
                    raise NotImplementedError("Eltwise SUM backward accumulating into a channel slice (%s)" % l.name)
                run = lambda st, a=gtop, b=gb: L.check(lib.fcn_eltwise_fwd_f32(a.ptr, b.ptr, b.ptr, a.pixels * a.cstride, L.ELT_SUM, 1.0, 1.0, st))
            else:
                run = lambda st, a=gtop, b=gb: L.check(lib.fcn_copy_channels_f32(
                    a.buf.ptr, b.buf.ptr, a.pixels, a.channels, a.cstride, a.coffset, b.cstride, b.coffset, st))
            self.ops.append(Op("eltwise_bwd", l.name + ":" + bn, run))
            self.mark(gb)

    def _deconvolution(self, l: Layer) -> None:
        if self.e.param_segs[(l.name, 0)].kind != S.DECONV:
            return self._one_bottom(l)
        gtop = self._arrived(l)
        if gtop is not None:
            self._dense_deconv(l, gtop, self.G.get(l.bottoms[0]))

    def _dense_deconv(self, l: Layer, gtop: Blob, gbot: Optional[Blob]) -> None:
        """Backward of a group-1 Deconvolution whose blob is kept as [Cin][kh][kw][Cout4], an OHWI bank of Cin outputs:
        db = per-channel sum of dY; dW = the weight-gradient kernel with the roles swapped (its x is dY, its y the layer's input);
        dX = the forward convolution of dY at the layer's stride."""
        e, lib, xb = self.e, self.lib, self.B[l.bottoms[0]]
        g = e._geom(l)
        co = g.cout
        if gtop.coffset % 4 or gtop.cstride % 4 or gtop.cstride - gtop.coffset < _r4(co):
            raise NotImplementedError("gradient view of %s is not a 16-byte aligned run of whole channel groups" % l.tops[0])
        gs = g.swapped()._replace(cin=_r4(co))
        flops = 2.0 * g.n * g.cin * g.h * g.w * co * g.k * g.k
        if e._learns(l) and l.name not in self.wgrad_done:
            if len(e.params_dev[l.name]) > 1:
                db = e._grad_view(l.name, 1)
                self.ops.append(Op("channel_sum", l.name, lambda st: L.check(lib.fcn_channel_sum_f32(
                    gtop.buf.ptr, db.ptr, gtop.pixels, co, gtop.cstride, gtop.coffset, st)), 0.0, 4.0 * gtop.pixels * co))
            if xb.coffset % 4 or xb.cstride % 4:
                raise NotImplementedError("input view of %s is not 16-byte aligned" % l.name)
            d = conv_desc(gtop, xb, gs)
            e._keep.append(d)
            self.wgrad_op(l.name, d, e._grad_view(l.name, 0), None, flops)
        if gbot is not None:
            d = conv_desc(gtop, gbot, gs, e.params_dev[l.name][0].ptr, flags=L.CONV_ACCUM if self.state(gbot) == "full" else 0)
            e._keep.append(d)
            self.mark(gbot, self.emit_dgrads(l.name, [(d, flops)], [l.bottoms[0]]))

    # ------------------------------------------------------------------ BatchNorm / Scale / ReLU chains
    def _batchnorm(self, l: Layer) -> None:
        """Backward of the chain that starts at l (engine._bn_chain_after; a Scale or ReLU absorbed into a chain has no entry and emits
        nothing): one reduce launch - sum dy' and sum dy' x-hat per channel, dy' = dY under the chain's ReLU mask - and one apply launch
        dX (+)= gamma invstd (dy' - sum dy' / m - x-hat sum dy' x-hat / m).  With a Scale the two sums ARE d(beta) and d(gamma) and go
        straight to its gradient views; the launch is on the main stream (it shares the forward's workspace) and names its layer, so
        the data-parallel exchange of that bucket waits for it.  With global statistics (a frozen BatchNorm) and for Scale alone the
        apply launch degenerates to dX (+)= gamma invstd dy', and the reduce launch runs only for a Scale that learns."""
        e, lib, B, G = self.e, self.lib, self.B, self.G
        ch = e._bn_chains.get(l.name)
        if ch is None:
            return
        gtop = G.get(ch.y)
        if gtop is None or self.state(gtop) == "none":
            return
        gbot = G.get(ch.x)
        xb, yb = B[ch.x], B[ch.y]
        pix, c = xb.pixels, xb.channels
        for g in (gtop, gbot):
            if g is not None and (g.coffset % 4 or g.cstride % 4):
                raise NotImplementedError("backward of %s %s: a gradient view that is not 16-byte aligned" % (l.type, l.name))
        aux = e.aux_dev.get(l.name)
        if aux is not None:
            hat = (aux.ptr, _r4(c), 0)
        elif ch.bn is None:
            hat = (xb.buf.ptr, xb.cstride, xb.coffset)      # Scale alone, not in place: its input is still there
        else:
            raise RuntimeError("BatchNorm %s kept no x-hat for its backward pass" % l.name)
        mask = (yb.buf.ptr, yb.cstride, yb.coffset) if ch.relu is not None else (None, 0, 0)
        learns = ch.scale is not None and e._learns(ch.scale) and ch.scale.name not in self.wgrad_done
        centred = ch.bn is not None and not ch.global_stats
        sums = (None, None)
        booked = None      # the launch the exchange of the Scale's bucket waits for: the LAST one that touches its gradient views
        if learns or (centred and gbot is not None):
            if ch.save is None:      # (Scale alone: nothing was saved in the forward pass)
                ch.save = DeviceBuffer(4 * _r4(c) * 4, zero=True)
                e._keep.append(ch.save)
            dbeta, dgamma = ch.save.ptr + 8 * _r4(c), ch.save.ptr + 12 * _r4(c)
            if learns:
                dgamma = e._grad_view(ch.scale.name, 0).ptr
                if len(e.params_dev[ch.scale.name]) > 1:      # (without a bias blob the sum of dy' has no gradient view to go to)
                    dbeta = e._grad_view(ch.scale.name, 1).ptr
                self.wgrad_done.add(ch.scale.name)
            booked = Op("bn_bwd_reduce", l.name, lambda st: L.check(lib.fcn_batchnorm_bwd_reduce_f32(
                gtop.buf.ptr, hat[0], mask[0], pix, c, gtop.cstride, gtop.coffset, hat[1], hat[2], mask[1], mask[2], dbeta, dgamma,
                e._bn_ws.ptr, st)), 3.0 * pix * c, (8.0 + (4.0 if mask[0] else 0.0)) * pix * c)
            self.ops.append(booked)
            if centred:
                sums = (dbeta, dgamma)
        if gbot is None:
            if learns:
                booked.layers = [ch.scale.name]
            return
        acc = 1 if self.state(gbot) == "full" and gbot is not gtop else 0
        save = ch.save.ptr if centred else None
        bvar, bfac, eps = None, None, 0.0
        if ch.bn is not None:
            eps = float(ch.bn.sub("batch_norm_param").get("eps", 1e-5))
            if not centred:
                bvar, bfac = e.params_dev[ch.bn.name][1].ptr, e.params_dev[ch.bn.name][2].ptr
        gamma = e.params_dev[ch.scale.name][0].ptr if ch.scale is not None else None
        self.ops.append(Op("bn_bwd_apply", l.name, lambda st: L.check(lib.fcn_batchnorm_bwd_apply_f32(
            gtop.buf.ptr, hat[0] if centred else None, mask[0], gbot.buf.ptr, pix, c, gtop.cstride, gtop.coffset, hat[1], hat[2], mask[1], mask[2],
            gbot.cstride, gbot.coffset, save, bvar, bfac, eps, gamma, sums[0], sums[1], acc, st)),
            4.0 * pix * c, (8.0 + (4.0 if centred else 0.0) + (4.0 if mask[0] else 0.0) + 4.0 * acc) * pix * c))
        if learns:      # (the apply launch reads the two sums where the reduce launch left them: the exchange must not sum them before)
            self.ops[-1].layers = [ch.scale.name]
        self.mark(gbot)

    # ------------------------------------------------------------------ gated Scale (the multiplier is a blob of the net)
    def _scale_gate(self, l: Layer) -> None:
        """Backward of a Scale with two bottoms (x, gate) - engine._scale_gate_op; TRAIN engines never fuse it: dx (+)= dY * gate[n, c] into
        G[x] and dgate[n, c] (+)= sum over the image's pixels of dY * x into G[gate], each accumulating where its view already holds a
        gradient and left out where that bottom needs none.  The data gradient comes first: in an SE block the global pooling's backward
        then accumulates into G[x].  One workspace, sized here, serves every gate gradient of the net (they run one after the other on
        the main stream)."""
        gtop = self._arrived(l)
        if gtop is None:
            return
        e, lib, B = self.e, self.lib, self.B
        xb, gb = B[l.bottoms[0]], B[l.bottoms[1]]
        n, ppi, c = scale_gate_form(l, [e.shapes[b] for b in l.bottoms], self.spec.phase)
        gx, gg = self.G.get(l.bottoms[0]), self.G.get(l.bottoms[1])
        for v in (gtop, gx, xb):
            if v is not None and (v.coffset % 4 or v.cstride % 4):
                raise NotImplementedError("backward of Scale %s: the view of %s is not 16-byte aligned" % (l.name, v.name))
        if gx is not None:
            acc_x = 1 if self.state(gx) == "full" else 0      # (a name of its own: the launch reads it when it runs, after the gate's is set)
            self.ops.append(Op("scale_gate_bwd", l.name + ":" + l.bottoms[0], lambda st: L.check(lib.fcn_scale_gate_bwd_data_f32(
                gtop.buf.ptr, gb.ptr, gx.buf.ptr, n, ppi, c, gtop.cstride, gtop.coffset, gb.cstride, gx.cstride, gx.coffset, acc_x, st)),
                1.0 * n * ppi * c, 4.0 * (2 + acc_x) * n * ppi * c))
            self.mark(gx)
        if gg is not None:
            acc_g = 1 if self.state(gg) == "full" else 0
            self.gate_ws_bytes = max(self.gate_ws_bytes, int(lib.fcn_scale_gate_workspace_bytes(n, ppi, c)))
            self.ops.append(Op("scale_gate_bwd", l.name + ":" + l.bottoms[1], lambda st: L.check(lib.fcn_scale_gate_bwd_gate_f32(
                gtop.buf.ptr, xb.buf.ptr, gg.ptr, n, ppi, c, gtop.cstride, gtop.coffset, xb.cstride, xb.coffset, gg.cstride, acc_g,
                e._gate_ws.ptr, st)), 2.0 * n * ppi * c, 8.0 * n * ppi * c))
            self.mark(gg)

    # ------------------------------------------------------------------ one bottom, one top, one launch dY -> dX
    def _one_bottom(self, l: Layer) -> None:
        gtop = self._arrived(l)
        gbot = self.G.get(l.bottoms[0]) if gtop is not None and l.bottoms else None
        act = self.activations.get(l.type) if l.type not in self.one_bottom else None
        if gbot is None and (act is None or gtop is None):      # (a PReLU or Bias may learn where its bottom needs no gradient)
            return
        # an in-place layer (bottom == top: drop6 / drop7 of the published FCN nets, an unfused in-place Sigmoid, ReLU or LRN) rewrites dY
        # as dX - there is nothing to accumulate into, whatever the layer type; `+=` into its own dY would be dY + f(dY)
        acc = 1 if gbot is not None and self.state(gbot) == "full" and gbot is not gtop else 0
        emit = self.one_bottom.get(l.type) or act or self.neurons.get(l.type) or self.shuffles.get(l.type)
        if emit is None:
            raise NotImplementedError("backward of layer type %s (%s)" % (l.type, l.name))
        emit(l, gtop, gbot, acc)

    def _chan_group_aligned(self, l: Layer, *views: Optional[Blob]) -> None:
        for v in views:
            if v is not None and (v.coffset % 4 or v.cstride % 4):
                raise NotImplementedError("backward of %s %s: the view of %s is not 16-byte aligned" % (l.type, l.name, v.name))

    def _ref_input(self, l: Layer, xb: Blob):
        """(pointer, cstride, coffset) of the layer's input as its data gradient reads it: the copy that the forward launch kept where
        the layer ran in place (engine._kept_input), else the bottom's view."""
        aux = self.e.aux_dev.get(l.name)
        if aux is not None:
            return aux.ptr, _r4(xb.channels), 0
        if l.tops[0] == l.bottoms[0]:
            raise RuntimeError("%s %s ran in place and kept no copy of its input for the backward pass" % (l.type, l.name))
        return xb.buf.ptr, xb.cstride, xb.coffset

    def _act(self, l: Layer, gtop: Blob, gbot: Optional[Blob], acc: int) -> None:
        """PReLU, TanH and Bias (csrc/act.hip, engine._fwd_act).  Where the layer's blob learns, the parameter-gradient launch comes first
        - in place the data launch rewrites the dY it reads - and overwrites that blob's segment of the flat gradient buffer; the data
        launch dX (+)= f'(ref) dY follows and is left out where the bottom needs no gradient.  ref is the layer's input for a PReLU (the
        copy the forward launch kept where the layer ran in place) and its output for a TanH.  One workspace, sized here, serves every
        parameter gradient of the net (they run one after the other on the main stream)."""
        e, lib, B, t = self.e, self.lib, self.B, l.type
        xb, yb = B[l.bottoms[0]], B[l.tops[0]]
        pix, c, mode = xb.pixels, xb.channels, L.ACT_MODES[t]
        self._chan_group_aligned(l, gtop, gbot, xb, yb)
        ref = (None, 0, 0)
        if t == "PReLU":
            ref = self._ref_input(l, xb)
        elif t == "TanH":
            ref = (yb.buf.ptr, yb.cstride, yb.coffset)
        param = e.params_dev[l.name][0].ptr if t == "PReLU" else None      # (the data gradient of a Bias reads no parameter)
        shared = int(t == "PReLU" and tuple(self.spec.param_shapes[l.name][0]) == ())
        if t != "TanH" and e._learns(l) and l.name not in self.wgrad_done:
            dparam = e._grad_view(l.name, 0).ptr
            self.act_ws_bytes = max(self.act_ws_bytes, int(lib.fcn_act_workspace_bytes(pix, c)))
            self.ops.append(Op("act_bwd_param", l.name, lambda st: L.check(lib.fcn_act_bwd_param_f32(
                gtop.buf.ptr, ref[0], dparam, pix, c, gtop.cstride, gtop.coffset, ref[1], ref[2], mode, shared, e._act_ws.ptr, st)),
                2.0 * pix * c, (8.0 if t == "PReLU" else 4.0) * pix * c))
            self.ops[-1].layers = [l.name]
            self.wgrad_done.add(l.name)
        if gbot is None:
            return
        self.ops.append(Op("act_bwd", l.name, lambda st: L.check(lib.fcn_act_bwd_data_f32(
            gtop.buf.ptr, ref[0], gbot.buf.ptr, pix, c, gtop.cstride, gtop.coffset, ref[1], ref[2], gbot.cstride, gbot.coffset, mode, param,
            shared, acc, st)), 1.0 * pix * c, 4.0 * ((2 if t == "Bias" else 3) + acc) * pix * c))
        self.mark(gbot)

    def _neuron(self, l: Layer, gtop: Blob, gbot: Blob, acc: int) -> None:
        """ELU, ReLU6, Clip, AbsVal, BNLL and Swish (csrc/neuron.hip, engine._fwd_neuron): one launch dX (+)= f'(ref) dY.  ref is the layer's
        output for ELU, ReLU6, Clip and BNLL - in place they need no copy -, its input for AbsVal (never in place) and for Swish (the copy
        the forward launch kept where the layer ran in place)."""
        lib, B, t = self.lib, self.B, l.type
        xb, yb = B[l.bottoms[0]], B[l.tops[0]]
        pix, c = xb.pixels, xb.channels
        mode, a, b = neuron_params(l)
        self._chan_group_aligned(l, gtop, gbot, xb, yb)
        if t == "Swish":
            ref = self._ref_input(l, xb)
        elif t == "AbsVal":
            ref = (xb.buf.ptr, xb.cstride, xb.coffset)
        else:
            ref = (yb.buf.ptr, yb.cstride, yb.coffset)
        self.ops.append(Op("neuron_bwd", l.name, lambda st: L.check(lib.fcn_neuron_bwd_f32(
            gtop.buf.ptr, ref[0], gbot.buf.ptr, pix, c, gtop.cstride, gtop.coffset, ref[1], ref[2], gbot.cstride, gbot.coffset, mode, a, b,
            acc, st)), 1.0 * pix * c, 4.0 * (3 + acc) * pix * c))
        self.mark(gbot)

    def _shuffle(self, l: Layer, gtop: Blob, gbot: Blob, acc: int) -> None:
        """ShuffleChannel (csrc/shuffle.hip, engine._fwd_shuffle): the gradient is the inverse permutation, the forward launch with group
        C / g: dX[i * (C / g) + j] (+)= dY[j * g + i].  No workspace, no kept input."""
        lib, xb = self.lib, self.B[l.bottoms[0]]
        pix, c = xb.pixels, xb.channels
        inv = c // shuffle_group(l, [xb.shape])
        self._chan_group_aligned(l, gtop, gbot)
        self.ops.append(Op("shuffle_bwd", l.name, lambda st: L.check(lib.fcn_shuffle_channel_f32(
            gtop.buf.ptr, gbot.buf.ptr, pix, c, inv, gtop.cstride, gtop.coffset, gbot.cstride, gbot.coffset, acc, st)),
            0.0, 4.0 * (2 + acc) * pix * c))
        self.mark(gbot)

    def _pooling(self, l: Layer, gtop: Blob, gbot: Blob, acc: int) -> None:
        pp = l.sub("pooling_param")
        if str(pp.get("pool", "MAX")) == "AVE":
            return self._ave_pooling(l, gtop, gbot, acc, bool(pp.get("global_pooling", False)))
        if str(pp.get("pool", "MAX")) != "MAX":
            raise NotImplementedError("backward of %s pooling (%s)" % (pp.get("pool"), l.name))
        g, lib, idx = self.e._geom(l), self.lib, self.e.aux_dev[l.name]
        rec = PoolBwd(l.bottoms[0])      # _finish_dgrads may fold a ReLU backward into this pass
        self.ops.append(Op("maxpool_bwd", l.name, lambda st: L.check(lib.fcn_maxpool_bwd_mask_f32(
            gtop.buf.ptr, idx.ptr, gbot.buf.ptr, g.n, g.h, g.w, g.cin, gbot.cstride, gbot.coffset, g.k, g.s, g.pad, g.oh, g.ow,
            gtop.cstride, gtop.coffset, acc, rec.mask[0], rec.mask[1], rec.mask[2], st))))
        self.mark(gbot, rec)

    def _ave_pooling(self, l: Layer, gtop: Blob, gbot: Blob, acc: int, global_pooling: bool) -> None:
        """fcn_avepool_bwd_f32: a gather, one lane per 16-byte channel group of a dX pixel (global pooling: the forward's k = H, stride 1)."""
        g, lib = self.e._geom(l, (gbot.shape[2], 1, 0) if global_pooling else None), self.lib
        if gtop.coffset % 4 or gtop.cstride % 4 or gbot.coffset % 4 or gbot.cstride % 4:
            raise NotImplementedError("backward of AVE pooling %s: a gradient view that is not 16-byte aligned" % l.name)
        self.ops.append(Op("avepool_bwd", l.name, lambda st: L.check(lib.fcn_avepool_bwd_f32(
            gtop.buf.ptr, gbot.buf.ptr, g.n, g.h, g.w, g.cin, gbot.cstride, gbot.coffset, g.k, g.s, g.pad, g.oh, g.ow,
            gtop.cstride, gtop.coffset, acc, st)), 0.0, 4.0 * (gtop.pixels + gbot.pixels * (1 + acc)) * g.cin))
        self.mark(gbot)

    def _crop(self, l: Layer, gtop: Blob, gbot: Blob, acc: int) -> None:
        """dX of bottom 0: dY inside the window and zeros outside in one launch, or += dY inside it when dX already holds a gradient.
        Bottom 1 lent its shape: no gradient goes there."""
        lib = self.lib
        _, (_, oc, oy, ox) = crop_window(l, self.B[l.bottoms[0]].shape, self.B[l.bottoms[1]].shape)
        if oc or gbot.channels != gtop.channels:
            raise NotImplementedError("backward of Crop %s along the channel axis" % l.name)
        n, c, h, w = gbot.shape
        _, _, oh, ow = gtop.shape
        self.ops.append(Op("crop_bwd", l.name, lambda st: L.check(lib.fcn_crop_bwd_f32(
            gtop.buf.ptr, gbot.buf.ptr, n, h, w, c, gbot.cstride, gbot.coffset, oy, ox, oh, ow, gtop.cstride, gtop.coffset, acc, st)),
            0.0, 4.0 * (gtop.pixels + gbot.pixels) * c))
        self.mark(gbot)

    def _interp(self, l: Layer, gtop: Blob, gbot: Blob, acc: int) -> None:
        """fcn_interp_bwd_f32: a gather, one lane per 16-byte channel group of a dX pixel; one launch writes all of dX (zeros where the
        pads crop or a shrink never reads), or adds into it when dX already holds a gradient."""
        lib = self.lib
        n, c, h, w = gbot.shape
        oh, ow, pad_beg, pad_end = interp_size(l, h, w)
        self.ops.append(Op("interp_bwd", l.name, lambda st: L.check(lib.fcn_interp_bwd_f32(
            gtop.buf.ptr, gbot.buf.ptr, n, h, w, c, gbot.cstride, gbot.coffset, pad_beg, pad_end, oh, ow, gtop.cstride, gtop.coffset, acc, st)),
            0.0, 4.0 * (gtop.pixels + gbot.pixels * (1 + acc)) * c))
        self.mark(gbot)

    def _upsample(self, l: Layer, gtop: Blob, gbot: Blob, acc: int) -> None:
        """fcn_unpool_bwd_f32: dX of bottom 0 gathers dY at the pixels the mask names.  Bottom 1 is the mask: no gradient goes there."""
        lib = self.lib
        pool = self.spec.mask_blobs[l.bottoms[1]]
        idx = self.e.aux_dev[pool.name]
        k, s, pad = kernel_stride_pad(pool.sub("pooling_param"))
        n, c, ph, pw = gbot.shape
        _, _, h, w = gtop.shape
        self.ops.append(Op("unpool_bwd", l.name, lambda st: L.check(lib.fcn_unpool_bwd_f32(
            gtop.buf.ptr, idx.ptr, gbot.buf.ptr, n, ph, pw, c, gbot.cstride, gbot.coffset, k, s, pad, h, w, gtop.cstride, gtop.coffset, acc, st)),
            0.0, 4.0 * gbot.pixels * c * (3 + acc)))
        self.mark(gbot)

    def _lrn(self, l: Layer, gtop: Blob, gbot: Blob, acc: int) -> None:
        xb, yb = self.B[l.bottoms[0]], self.B[l.tops[0]]
        p = l.sub("lrn_param")
        ls, al, be = int(p.get("local_size", 5)), float(p.get("alpha", 1.0)), float(p.get("beta", 0.75))
        lib, sc = self.lib, self.e.aux_dev[l.name]
        if gtop.coffset or gbot.coffset or xb.coffset or yb.coffset:
            raise NotImplementedError("LRN backward on channel slices (%s)" % l.name)
        self.ops.append(Op("lrn_bwd", l.name, lambda st: L.check(lib.fcn_lrn_bwd_f32(
            xb.ptr, yb.ptr, sc.ptr, gtop.ptr, gbot.ptr, xb.pixels, xb.channels, xb.cstride, yb.cstride, ls, al, be, acc, st))))
        self.mark(gbot)

    def _dropout(self, l: Layer, gtop: Blob, gbot: Blob, acc: int) -> None:
        if acc:
            raise NotImplementedError("dropout backward into an already written gradient (%s)" % l.name)
        e, lib = self.e, self.lib
        ratio = float(l.sub("dropout_param").get("dropout_ratio", 0.5))
        n, c, h, w = self.B[l.bottoms[0]].nchw
        salt = dropout_layer_salt(self.spec, l)      # the mask the forward launch of this layer drew
        self.ops.append(Op("dropout_bwd", l.name, lambda st: L.check(lib.fcn_dropout_f32(
            gtop.buf.ptr, gbot.buf.ptr, n, c, h, w, gtop.cstride, gtop.coffset, gbot.cstride, gbot.coffset, ratio,
            (e.dropout_seed + salt) & 0xFFFFFFFF, e.dropout_index_offset, st))))
        self.mark(gbot)

    def _eltwise_prod(self, l: Layer, gtop: Blob, gbot: Blob, acc: int) -> None:
        opname = str(l.sub("eltwise_param").get("operation", "SUM"))
        if opname != "PROD" or len(l.bottoms) != 2:
            raise NotImplementedError("backward of Eltwise %s" % l.name)
        if l.bottoms[1] in self.e.need_grad:
            raise NotImplementedError("Eltwise PROD backward w.r.t. both bottoms (%s)" % l.name)
        if acc:
            raise NotImplementedError("Eltwise backward into an already written gradient (%s)" % l.name)
        lib, other = self.lib, self.B[l.bottoms[1]]
        count = gtop.pixels * gtop.cstride
        if gtop.coffset or gbot.coffset or other.coffset or other.cstride != gtop.cstride:
            raise NotImplementedError("Eltwise backward on channel slices")
        self.ops.append(Op("eltwise_bwd", l.name, lambda st: L.check(lib.fcn_eltwise_fwd_f32(
            gtop.ptr, other.ptr, gbot.ptr, count, L.ELT_PROD, 1.0, 1.0, st))))
        self.mark(gbot)

    def _depthwise_deconv(self, l: Layer, gtop: Blob, gbot: Blob, acc: int) -> None:
        if any(m != 0.0 for m in l.lr_mult) or not l.lr_mult:
            raise NotImplementedError("learnable depthwise Deconvolution %s (group == channels): only group 1 learns; the reference "
                                      "freezes its bilinear upsampling, lr_mult 0" % l.name)
        g, lib = self.e._geom(l), self.lib
        wdev = self.e.params_dev[l.name][0].ptr
        self.ops.append(Op("deconv_bwd", l.name, lambda st: L.check(lib.fcn_deconv_depthwise_bwd_f32(
            gtop.buf.ptr, wdev, gbot.ptr, g.n, g.h, g.w, g.cin, gbot.cstride, g.k, g.s, g.pad, g.oh, g.ow, gtop.cstride, gtop.coffset, acc, st))))
        self.mark(gbot)

    def _sigmoid_plain(self, l: Layer, gtop: Blob, gbot: Blob, acc: int) -> None:
        lib, yb = self.lib, self.B[l.tops[0]]
        self.ops.append(Op("sigmoid_bwd", l.name, lambda st: L.check(lib.fcn_sigmoid_bwd_f32(
            yb.ptr, gtop.ptr, gbot.ptr, yb.pixels * yb.cstride, acc, st))))
        self.mark(gbot)

    def _relu_plain(self, l: Layer, gtop: Blob, gbot: Blob, acc: int) -> None:
        """A ReLU layer of its own (engine._relu_after and _bn_chain_after leave every ReLU with a slope to this one): dX (+)= dY where the
        output is positive and negative_slope dY elsewhere.  The stored output stands in for the input - their signs agree for a slope
        >= 0, in place too; below 0 they do not, and nothing here keeps the input."""
        lib, yb = self.lib, self.B[l.tops[0]]
        slope = float(l.sub("relu_param").get("negative_slope", 0.0))
        if slope < 0.0:
            raise NotImplementedError("ReLU %s: backward with negative_slope %g (below 0 the sign of the output is not the sign of the input)"
                                      % (l.name, slope))
        self.ops.append(Op("relu_bwd", l.name, lambda st: L.check(lib.fcn_relu_bwd_slope_f32(
            gtop.ptr, yb.ptr, gbot.ptr, yb.pixels, yb.channels, yb.cstride, slope, acc, st))))
        self.mark(gbot)
