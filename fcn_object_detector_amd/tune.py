"""Plan-time autotuner: what an engine times on the device while it is built.

A :class:`Tuner` belongs to one engine.  It owns what timing needs (an event pair, the 64 MB buffer that evicts the L2s), the
decisions taken so far (`chosen`) and their copy in the $FCN_TUNE_CACHE file.  Everything timed goes through one primitive,
:meth:`Tuner.measure`; the three timing protocols are rows of :class:`Protocol`; every decision - a launch's tile
configuration, the cut of a half-float level, the level of an inception floater, a weight-gradient configuration - is taken
through :meth:`Tuner.choose`, which replays it from a replica's tuner or from the cache file before it searches.
"""
from __future__ import annotations

import ctypes as C
import json
import os
from typing import Callable, Dict, Iterable, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np

from . import engine as E
from . import lib as L


def lower_quartile(samples: Sequence[float]) -> float:
    return float(np.percentile(samples, 25))      # (disturbances only ever lengthen a launch: the lower quartile, not the median)


class Protocol(NamedTuple):
    """How a set of configurations is ranked.  First pass, per configuration: `warm` untimed launches, then `samples` windows of
    `reps` launches (each after an eviction of the L2s if `evict`), summarised by `stat`.  Second look: the `contenders` fastest
    within `margin` of the fastest get `look` more windows each; `stat` over them (and the first-pass figure, if `carry`) decides."""
    warm: int
    reps: int
    evict: bool
    samples: int
    stat: Callable[[Sequence[float]], float]
    contenders: int
    margin: float
    look: int
    carry: bool


# Cold timing (round 4, $FCN_TUNE_COLD=0 for the old way): inside a forward pass a launch finds its filters in HBM / the Infinity
# Cache, not in L2 - 24 MB of filters and ~250 MB of activations pass through the 4 MB L2s between two frames - but six
# repetitions of ONE launch back to back are warm from the second on, which favours the configurations that tolerate memory
# latency worst (rocprofv3's durations of whole forwards were 4-5 % longer than the back-to-back ones).  So every timed launch is
# preceded by a pass over a 64 MB scratch buffer that evicts the L2s; the event pair's own cost is the same for every
# configuration and leaves the ranking alone.  The one untimed launch loads the code object and the kernel arguments.
# (tried, round 4: the plan's previous launch between the eviction and the timed launch, so that the inputs sit where a forward leaves
#  them - the chosen plans ran the frame in the same 0.2736 - 0.2743 ms)
# Its second look (round 4): the first pass's lower quartile of seven separates configurations that differ by 2 % or more; two that
# differ by less are a coin toss there, and the plan of a 20-launch net then moves by half a per cent from run to run.  The four
# fastest within 5 % are timed again, 31 cold launches each, and the smallest lower quartile wins.
COLD = Protocol(warm=1, reps=1, evict=True, samples=7, stat=lower_quartile, contenders=4, margin=1.05, look=31, carry=False)
# Back to back (TRAIN-phase engines, and every engine under FCN_TUNE_COLD=0): the same second look, five more rounds of six launches, the minimum
WARM = Protocol(warm=2, reps=6, evict=False, samples=1, stat=min, contenders=3, margin=1.04, look=5, carry=True)
# Weight gradients: as WARM, four more rounds of five launches each
WGRAD = Protocol(warm=2, reps=5, evict=False, samples=1, stat=min, contenders=3, margin=1.04, look=4, carry=True)

FLUSH_BYTES = 64 << 20


def set_partitions(n: int) -> Iterable[List[int]]:
    """The set partitions of n items as restricted-growth label lists ([0, 0, 1]: the third item in a group of its own)."""
    def rec(labels: List[int], groups: int):
        if len(labels) == n:
            yield list(labels)
            return
        for g in range(groups + 1):
            labels.append(g)
            yield from rec(labels, max(groups, g + 1))
            labels.pop()
    yield from rec([], 0)


def key_suffix(input_shape: Optional[Sequence[int]], f16: bool, max_lds: int) -> str:
    """What follows a decision's name in its cache key: the shape of the net's first input (None: a net without inputs), the
    number format and the LDS cap if there is one."""
    key = "|" + ("x".join(str(d) for d in input_shape) if input_shape is not None else "")
    return key + ("|f16" if f16 else "") + ("|lds%d" % (max_lds // 1024) if max_lds < 160 * 1024 else "")


class Tuner:
    def __init__(self, stream: int, key_suffix: str, cold: bool, max_lds: int, tune_from: Optional[Dict[str, object]] = None):
        """stream: the engine's; key_suffix: what tells this engine's decisions from another's in the cache file ("|1x3x384x1248|f16");
        cold: a TEST-phase engine; max_lds: the LDS cap on tile configurations, bytes; tune_from: `chosen` of a replica of the
        same net, whose plan is reused instead of timing again."""
        self.stream, self.key_suffix, self.cold, self.max_lds, self.tune_from = stream, key_suffix, cold, max_lds, tune_from
        self.chosen: Dict[str, object] = {}      # decision key -> tile configuration (int) or cut / move code (str)
        self.events: Optional[Tuple[C.c_void_p, C.c_void_p]] = None
        self.flush: Optional["E.DeviceBuffer"] = None
        self.cache_path = os.environ.get("FCN_TUNE_CACHE") or None
        self.cache: Optional[dict] = None
        if self.cache_path:
            try:
                with open(self.cache_path) as f:
                    self.cache = json.load(f)
            except (OSError, ValueError):
                self.cache = {}
            if not isinstance(self.cache, dict):
                self.cache = {}

    def key(self, name: str) -> str:
        return name + self.key_suffix

    def release(self) -> None:
        """Destroys the event pair and frees the eviction buffer: nothing of the tuner's is alive when the next replica of a
        pipeline is built.  Safe to call again; a later measurement makes what it needs anew."""
        if self.events is not None:
            for ev in self.events:
                L.call("fcn_event_destroy", ev)
            self.events = None
        if self.flush is not None:
            self.flush.free()
            self.flush = None

    # ------------------------------------------------------------------ timing
    def measure(self, launch: Callable[[], None], reps: int, evict: bool = False) -> float:
        """Milliseconds per launch of `reps` launches issued back to back between two events, after a pass over the eviction
        buffer if `evict`."""
        if self.events is None:
            e0, e1 = C.c_void_p(), C.c_void_p()
            L.call("fcn_event_create", C.byref(e0))
            L.call("fcn_event_create", C.byref(e1))
            self.events = (e0, e1)
        e0, e1 = self.events
        if evict:
            if self.flush is None:
                self.flush = E.DeviceBuffer(FLUSH_BYTES, zero=False)
            L.call("fcn_memset_async", self.flush.ptr, 0, self.flush.nbytes, self.stream)
        L.call("fcn_event_record", e0, self.stream)
        for _ in range(reps):
            launch()
        L.call("fcn_event_record", e1, self.stream)
        L.call("fcn_event_sync", e1)
        ms = C.c_float()
        L.call("fcn_event_elapsed_ms", e0, e1, C.byref(ms))
        return ms.value / reps

    def fastest(self, cfgs: Iterable[int], prepare: Callable[[int], bool], launch: Callable[[], None], p: Protocol,
                second_look: bool = True) -> Tuple[int, float]:
        """(fastest of `cfgs`, its milliseconds per launch) by protocol p; (-1, 1e30) if prepare() refuses them all."""
        timed: List[Tuple[float, int]] = []
        for cfg in cfgs:
            if not prepare(cfg):
                continue
            for _ in range(p.warm):
                launch()
            timed.append((p.stat([self.measure(launch, p.reps, p.evict) for _ in range(p.samples)]), cfg))
        if not timed:
            return -1, 1e30
        best_ms, best = min(timed)
        if second_look and len(timed) > 1:
            finals = []
            for t1, cfg in sorted(timed)[:p.contenders]:
                if t1 > p.margin * best_ms:
                    break
                if prepare(cfg):
                    finals.append((p.stat(([t1] if p.carry else []) + [self.measure(launch, p.reps, p.evict) for _ in range(p.look)]), cfg))
            if finals:
                best_ms, best = min(finals)
        return best, best_ms

    def time_conv_cfgs(self, arr, n: int, ws: "E.DeviceBuffer", parr=None, npool: int = 0) -> Tuple[int, float]:
        """(fastest tile configuration, its milliseconds per launch) of one grouped launch."""
        lib = L.load()
        grp = L.ConvGroup()
        first_layer = int(lib.fcn_conv2d_first_layer_config())
        cold = self.cold and os.environ.get("FCN_TUNE_COLD", "1") != "0"

        def admitted(cfg: int) -> bool:
            # (the LDS cap keeps the tiles of several frames in flight resident on one CU; the first-layer kernel puts one
            #  workgroup per CU and frame and is exempt)
            if cfg == first_layer:
                return os.environ.get("FCN_CONV_FIRST7", "1") != "0"
            return int(lib.fcn_conv2d_config_lds_bytes(cfg)) <= self.max_lds

        def prepare(cfg: int) -> bool:      # False: a configuration that does not take this group (the first-layer kernel is shape-specific)
            return lib.fcn_conv2d_group_prepare_fused(arr, n, parr, npool, ws.ptr, cfg, C.byref(grp)) == 0

        return self.fastest([c for c in range(int(lib.fcn_conv2d_num_configs())) if admitted(c)], prepare,
                            lambda: L.check(lib.fcn_conv2d_fwd_group_f32(C.byref(grp), self.stream)), COLD if cold else WARM,
                            cold or os.environ.get("FCN_TUNE_SECOND_LOOK", "1") != "0")

    def _subset_ms(self, descs: Sequence[L.ConvDesc], pools: Sequence[L.PoolDesc] = ()) -> float:
        """Milliseconds of the convolutions `descs` (and the poolings that ride) as one launch in its fastest configuration."""
        lib = L.load()
        arr = (L.ConvDesc * len(descs))(*descs)
        parr = (L.PoolDesc * max(len(pools), 1))(*pools) if pools else None
        ws = E.DeviceBuffer(int(lib.fcn_conv2d_group_workspace_bytes(len(descs))), zero=False)
        try:
            return self.time_conv_cfgs(arr, len(descs), ws, parr, len(pools))[1]
        finally:
            L.call("fcn_conv2d_group_release", ws.ptr)
            ws.free()

    # ------------------------------------------------------------------ decisions
    def choose(self, key: str, valid: Callable[[object], bool], search: Callable[[], object]):
        """The decision `key`: a replica's, else the cache file's, else search()'s - the first whose value is valid.  Remembered in
        `chosen`; a searched one also goes into the cache file (an unwritable file is ignored)."""
        for known in (self.tune_from, self.cache):
            if known is not None and valid(known.get(key)):
                value = known[key]
                break
        else:
            value = search()
            if self.cache is not None:
                self.cache[key] = value
                try:
                    with open(self.cache_path, "w") as f:
                        json.dump(self.cache, f, indent=0, sort_keys=True)
                except OSError:
                    pass
        self.chosen[key] = value
        return value

    @staticmethod
    def _valid_cfg(ncfg: int) -> Callable[[object], bool]:
        return lambda v: type(v) is int and 0 <= v < ncfg

    def conv_cfg(self, name: str, arr, n: int, ws: "E.DeviceBuffer", parr=None, npool: int = 0) -> int:
        """Autotuned tile configuration of one grouped launch (forward: `name` carries the {+N pool} / {+tail} decorations;
        data gradients: "dgrad:<...>")."""
        return self.choose(self.key(name), self._valid_cfg(int(L.load().fcn_conv2d_num_configs())),
                           lambda: self.time_conv_cfgs(arr, n, ws, parr, npool)[0])

    def wgrad_cfgs(self, ops: Sequence["E.Op"]) -> None:
        """Plan-time choice of every weight-gradient launch's configuration (the 64-wide tile shapes and the role-split kernel of
        csrc/train.hip): each is timed on the buffers the step will use and the fastest is kept.  Gradient buffers hold garbage until
        the first real backward pass, which overwrites them."""
        ncfg = int(L.load().fcn_conv2d_wgrad_num_configs())
        for op in ops:
            if op.kind != "wgrad" or op.sel is None:      # (an InnerProduct weight gradient has one form: nothing to choose)
                continue

            def select(cfg: int) -> bool:
                op.sel["cfg"] = cfg
                return True

            op.sel["cfg"] = self.choose(self.key("wgrad:" + "+".join(op.layers)), self._valid_cfg(ncfg),
                                        lambda: self.fastest(range(ncfg), select, lambda: op.run(self.stream), WGRAD)[0])
            op.name += " [cfg%d]" % op.sel["cfg"]

    def split_level(self, chunk: List["E.ConvTask"]) -> List[List["E.ConvTask"]]:
        """Half-float engines: which launches carry a level's convolutions?  The streaming kernel's configurations are shaped for one
        kind of problem or another (filter sizes, channel counts), so for the two to four convolutions of an inception level every way
        of cutting the level into launches is priced - each subset's fastest configuration is timed once - and the cheapest cut is
        kept (round 3; rounds 2-3a knew two cuts: one launch, or 3x3 / 5x5 beside 1x1).  The decision rides in the tune cache beside the
        configurations, as a string of group labels ("001": the third convolution has a launch of its own)."""
        n = len(chunk)
        if n < 2 or n > 4:
            return [chunk]

        def valid(code) -> bool:
            return isinstance(code, str) and len(code) == n and all(ch.isdigit() and int(ch) < n for ch in code)

        def search() -> str:
            memo: Dict[Tuple[int, ...], float] = {}

            def cost(sub: Tuple[int, ...]) -> float:
                if sub not in memo:
                    memo[sub] = self._subset_ms([chunk[i].desc for i in sub])
                return memo[sub]

            best, best_ms = None, 1e30
            for labels in set_partitions(n):
                ms = sum(cost(tuple(i for i in range(n) if labels[i] == g)) for g in sorted(set(labels)))
                if ms < best_ms - 1e-7:
                    best, best_ms = labels, ms
            return "".join(str(g) for g in best)

        choice = self.choose("cut|" + self.key("+".join(it.layer.name for it in chunk)), valid, search)
        groups: Dict[str, List[E.ConvTask]] = {}
        for it, g in zip(chunk, choice):
            groups.setdefault(g, []).append(it)
        return [groups[g] for g in sorted(groups)]

    def move_floaters(self, tasks: Sequence[object], levels: List[int]) -> None:
        """Float engines: which LEVEL carries a convolution that nobody waits for?  An inception module is two levels -
        {1x1, 3x3_reduce, 5x5_reduce} (+ the module's pooling) and {3x3, 5x5, pool_proj} - but the plain 1x1 branch is read by
        nothing before the NEXT module: it may ride in either launch.  In the first it makes a latency-bound launch wider (at
        28 x 28 the reduce level is one 32 x 32 tile per CU whichever way); in the second its short tiles fill the CUs beside the
        long 3x3 tiles.  Every placement of a level's floaters is priced - both launches with their fastest configurations, the
        lower of two timings - and the cheapest kept (round 4; the decision rides in the tune cache as a string of 0 / 1 per floater).
        Changes `levels` in place."""
        for lv in range(max(levels, default=-1)):
            a_idx, b_idx = ([i for i, t in enumerate(tasks) if levels[i] == l2 and isinstance(t, E.ConvTask)] for l2 in (lv, lv + 1))
            if len(a_idx) < 2 or not b_idx or len(a_idx) > 8:
                continue
            fl = [i for i in a_idx if E.task_floats(tasks, levels, i)]
            if not fl or len(fl) > 3 or len(b_idx) + len(fl) > 8:
                continue

            def valid(code) -> bool:      # (never everything out of a level)
                return isinstance(code, str) and len(code) == len(fl) and set(code) <= {"0", "1"} and (len(fl) < len(a_idx) or "0" in code)

            def search() -> str:
                pools = {l2: [t.pool_desc for j, t in enumerate(tasks) if levels[j] == l2 and isinstance(t, E.OpTask) and t.pool_desc is not None][:2]
                         for l2 in (lv, lv + 1)}
                memo: Dict[Tuple[int, Tuple[int, ...]], float] = {}

                def cost(l2: int, sub: Tuple[int, ...]) -> float:
                    if (l2, sub) not in memo:
                        memo[(l2, sub)] = min(self._subset_ms([tasks[i].desc for i in sub], pools[l2]) for _ in range(2))
                    return memo[(l2, sub)]

                best, best_ms, base_ms = "0" * len(fl), None, None
                for code in range(1 << len(fl)):
                    moved = [fl[b] for b in range(len(fl)) if code >> b & 1]
                    stay = tuple(i for i in a_idx if i not in moved)
                    if not stay:
                        continue
                    ms = cost(lv, stay) + cost(lv + 1, tuple(b_idx + moved))
                    if code == 0:
                        base_ms = ms
                    if best_ms is None or ms < best_ms:
                        best, best_ms = "".join("1" if code >> b & 1 else "0" for b in range(len(fl))), ms
                # (timing noise: a move must be worth 1 % of the pair - 3 % until the tuner took a second look at close contenders)
                if best_ms > float(os.environ.get("FCN_MOVE_MARGIN", "0.99")) * base_ms:
                    best = "0" * len(fl)
                return best

            names = ("+".join(tasks[i].layer.name for i in idx) for idx in (a_idx, b_idx))
            choice = self.choose("move|" + self.key(">".join(names)), valid, search)
            for b, i in enumerate(fl):
                if choice[b] == "1":
                    levels[i] = lv + 1
