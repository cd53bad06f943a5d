"""The plan-time autotuner (fcn_object_detector_amd/tune.py) driven without a device.

A fake library answers the entry points the tuner calls, keeps a device clock that every launch advances by a scripted number
of milliseconds, and counts launches, evictions, events and allocations.  What is asserted is the PROTOCOL: how often each
configuration is launched, which ones get a second look, who wins, what is replayed and what is written to the cache file.

Provenance of the literals: every scenario below that times something (the protocol, margin and admission cases, the
weight-gradient table, the cuts, the moves and their guards), the cache keys, the replays and the cache file's text were also run
against the methods this module replaced - Engine._time_conv_cfgs, _tune_key, _tuned_cfg, _split_level, _move_floaters and
TrainEngine._tune_wgrads of commit 365206e, called on a stub object with this fake library installed - and gave the same
launches per configuration, winners, evictions, allocations, keys, decision codes and file contents.  New with this module:
a cached configuration that is not an integer is searched again (the old code converted or raised), a replica's configuration
is validated, and release() destroys the events.
"""
import ctypes as C
import json
from collections import Counter
from types import SimpleNamespace

import pytest

from fcn_object_detector_amd import lib as L
from fcn_object_detector_amd import tune as T
from fcn_object_detector_amd.engine import ConvTask, Op, OpTask, task_floats, task_levels

SUFFIX = "|1x3x8x8"


class FakeLib:
    """`ms(problem, cfg, nth)` scripts the milliseconds of the nth launch (from 0) of configuration cfg on a problem: the tuple
    of the Cout fields of the descriptors last prepared, followed by the number of poolings that ride - or ("wgrad", name)."""

    def __init__(self, ms, ncfg=6, lds=None, first_layer=-1, refused=(), wgrad_ncfg=0):
        self.ms, self.ncfg, self.lds, self.first_layer, self.refused, self.wgrad_ncfg = ms, ncfg, lds or [0] * ncfg, first_layer, set(refused), wgrad_ncfg
        self.calls = Counter()           # entry point -> calls
        self.launches = Counter()        # (problem, cfg) -> launches
        self.clock, self.marks = 0.0, {}
        self.events_made, self.events_live = 0, set()
        self.allocs, self.alloc_sizes = {}, []
        self.evictions = 0
        self.current = None

    def __getattr__(self, name):         # only the entry points written out below exist: anything else the tuner called would fail here
        if not name.startswith("fcn_"):
            raise AttributeError(name)
        impl = object.__getattribute__(self, "_" + name)

        def counted(*args):
            self.calls[name] += 1
            return impl(*args)
        return counted

    def launch(self, problem, cfg):
        self.clock += self.ms(problem, cfg, self.launches[(problem, cfg)])
        self.launches[(problem, cfg)] += 1

    def per_cfg(self, problem):
        return [self.launches[(problem, c)] for c in range(max(self.ncfg, self.wgrad_ncfg))]

    @staticmethod
    def _h(e):
        return e.value if isinstance(e, C.c_void_p) else e

    def _fcn_event_create(self, ref):
        self.events_made += 1
        ref._obj.value = 0x1000 + self.events_made
        self.events_live.add(ref._obj.value)
        return 0

    def _fcn_event_destroy(self, e):
        self.events_live.remove(self._h(e))
        return 0

    def _fcn_event_record(self, e, stream):
        self.marks[self._h(e)] = self.clock
        return 0

    def _fcn_event_sync(self, e):
        return 0

    def _fcn_event_elapsed_ms(self, e0, e1, ref):
        ref._obj.value = self.marks[self._h(e1)] - self.marks[self._h(e0)]
        return 0

    def _fcn_malloc(self, ref, nbytes):
        ref._obj.value = 0x100000 * (len(self.alloc_sizes) + 1)
        self.allocs[ref._obj.value] = nbytes
        self.alloc_sizes.append(nbytes)
        return 0

    def _fcn_free(self, ptr):
        del self.allocs[ptr]
        return 0

    def _fcn_memset_async(self, ptr, value, nbytes, stream):
        assert self.allocs[ptr] == nbytes == 64 << 20
        self.evictions += 1
        return 0

    def _fcn_conv2d_num_configs(self):
        return self.ncfg

    def _fcn_conv2d_first_layer_config(self):
        return self.first_layer

    def _fcn_conv2d_config_lds_bytes(self, cfg):
        return self.lds[cfg]

    def _fcn_conv2d_group_workspace_bytes(self, n):
        return 256 * n

    def _fcn_conv2d_group_release(self, ptr):
        assert ptr in self.allocs
        return 0

    def _fcn_conv2d_group_prepare_fused(self, arr, n, parr, npool, ws, cfg, ref):
        if cfg in self.refused:
            return 1
        self.current = (tuple(arr[i].Cout for i in range(n)) + (npool,), cfg)
        return 0

    def _fcn_conv2d_fwd_group_f32(self, ref, stream):
        self.launch(*self.current)
        return 0

    def _fcn_conv2d_wgrad_num_configs(self):
        return self.wgrad_ncfg


def table(times):
    return lambda problem, cfg, nth: times[cfg]


@pytest.fixture
def install(monkeypatch):
    monkeypatch.delenv("FCN_TUNE_CACHE", raising=False)
    for v in ("FCN_TUNE_COLD", "FCN_TUNE_SECOND_LOOK", "FCN_CONV_FIRST7", "FCN_MOVE_MARGIN"):
        monkeypatch.delenv(v, raising=False)

    def _install(fake):
        monkeypatch.setattr(L, "_lib", fake)
        return fake
    return _install


def tuner(cold, max_lds=160 * 1024, tune_from=None):
    return T.Tuner(1, SUFFIX, cold, max_lds, tune_from)


def descs(*ids):
    out = []
    for i in ids:
        d = L.ConvDesc()
        d.Cout = i
        out.append(d)
    return out


def one_problem(tn, ident=7):
    ds = descs(ident)
    return tn.time_conv_cfgs((L.ConvDesc * 1)(*ds), 1, SimpleNamespace(ptr=0x40))


P7 = (7, 0)      # the problem one_problem() times: one descriptor, no pooling


# ------------------------------------------------------------------ the two protocols
TIMES_ISSUE = [1.0, 1.03, 1.2, 1.04, 1.049, 1.06]      # (1.04 sits on the back-to-back margin: used for the cold protocol only)


def test_cold_protocol(install):
    fake = install(FakeLib(table(TIMES_ISSUE)))
    tn = tuner(cold=True)
    best, ms = one_problem(tn)
    assert best == 0 and ms == pytest.approx(1.0, rel=1e-6)
    assert fake.per_cfg(P7) == [39, 39, 8, 39, 39, 8]      # 1 + 7 for everyone, + 31 for the four within 5 %
    assert fake.evictions == 166 and fake.alloc_sizes == [64 << 20]
    assert fake.events_made == 2


def test_back_to_back_protocol(install):
    fake = install(FakeLib(table([1.0, 1.03, 1.2, 1.035, 1.049, 1.06])))
    best, ms = one_problem(tuner(cold=False))
    assert best == 0 and ms == pytest.approx(1.0, rel=1e-6)
    assert fake.per_cfg(P7) == [38, 38, 8, 38, 8, 8]        # 2 + 6, then 5 x 6 for the three fastest (all within 4 %)
    assert fake.evictions == 0 and fake.alloc_sizes == []


def test_test_phase_engine_times_back_to_back_under_tune_cold_0(install, monkeypatch):
    monkeypatch.setenv("FCN_TUNE_COLD", "0")
    fake = install(FakeLib(table([1.0, 1.03, 1.2, 1.035, 1.049, 1.06])))
    assert one_problem(tuner(cold=True))[0] == 0
    assert fake.per_cfg(P7) == [38, 38, 8, 38, 8, 8] and fake.evictions == 0


@pytest.mark.parametrize("cold,third,want", [
    (True, 1.045, [39, 39, 39, 8]), (True, 1.055, [39, 39, 8, 8]),          # 5 %: just inside, just outside
    (False, 1.035, [38, 38, 38, 8]), (False, 1.045, [38, 38, 8, 8])])       # 4 %
def test_second_look_margin(install, cold, third, want):
    fake = install(FakeLib(table([1.0, 1.02, third, 1.5]), ncfg=4))
    assert one_problem(tuner(cold))[0] == 0
    assert fake.per_cfg(P7) == want


@pytest.mark.parametrize("cold,want", [(True, [39, 39, 39, 39, 8, 8]), (False, [38, 38, 38, 8, 8, 8])])
def test_second_look_contender_limit(install, cold, want):
    fake = install(FakeLib(table([1.0, 1.001, 1.002, 1.003, 1.004, 1.005])))      # all within the margin: four resp. three get the look
    assert one_problem(tuner(cold))[0] == 0
    assert fake.per_cfg(P7) == want


@pytest.mark.parametrize("cold,winner", [(True, 0), (False, 1)])
def test_second_look_decides(install, cold, winner):
    """Configuration 1 runs its first eight launches (the whole first pass of either protocol) in 0.99 ms and every later one in
    1.02.  Cold, the second look's 31 samples alone decide: 0 wins.  Back to back the first-pass figure stays among the rounds
    whose minimum counts: 1 keeps its 0.99."""
    fake = install(FakeLib(lambda problem, cfg, nth: [1.0, 0.99 if nth < 8 else 1.02, 1.5][cfg], ncfg=3))
    best, ms = one_problem(tuner(cold))
    assert best == winner and ms == pytest.approx([1.0, 0.99][winner], rel=1e-6)


def test_second_look_switch_is_for_back_to_back_only(install, monkeypatch):
    monkeypatch.setenv("FCN_TUNE_SECOND_LOOK", "0")
    fake = install(FakeLib(table([1.0, 1.01, 1.5]), ncfg=3))
    one_problem(tuner(cold=False))
    assert fake.per_cfg(P7) == [8, 8, 8]
    fake = install(FakeLib(table([1.0, 1.01, 1.5]), ncfg=3))
    one_problem(tuner(cold=True))
    assert fake.per_cfg(P7) == [39, 39, 8]


def test_single_configuration_gets_no_second_look(install):
    fake = install(FakeLib(table([1.0]), ncfg=1))
    assert one_problem(tuner(cold=True))[0] == 0 and fake.per_cfg(P7) == [8]


# ------------------------------------------------------------------ admission
def test_prepare_refusal(install):
    fake = install(FakeLib(table(TIMES_ISSUE), refused=[0]))
    assert one_problem(tuner(cold=False))[0] == 1
    assert fake.per_cfg(P7)[0] == 0 and fake.per_cfg(P7)[1] == 38


def test_nothing_admitted(install):
    fake = install(FakeLib(table([1.0, 1.0]), ncfg=2, refused=[0, 1]))
    assert one_problem(tuner(cold=False))[0] == -1 and not fake.launches


def test_lds_cap_exempts_the_first_layer_configuration(install, monkeypatch):
    lds = [64 << 10, 36 << 10, 160 << 10, 20 << 10]
    fake = install(FakeLib(table([1.0, 1.5, 0.5, 2.0]), ncfg=4, lds=lds, first_layer=2))
    assert one_problem(tuner(cold=False, max_lds=36 << 10))[0] == 2          # 0 is over the cap, 2 is too but is the first-layer kernel
    assert fake.per_cfg(P7) == [0, 8, 38, 8]
    fake = install(FakeLib(table([1.0, 1.5, 0.5, 2.0]), ncfg=4, lds=lds, first_layer=-1))
    assert one_problem(tuner(cold=False, max_lds=36 << 10))[0] == 1
    assert fake.per_cfg(P7) == [0, 38, 0, 8]
    monkeypatch.setenv("FCN_CONV_FIRST7", "0")
    fake = install(FakeLib(table([1.0, 1.5, 0.5, 2.0]), ncfg=4, lds=lds, first_layer=2))
    assert one_problem(tuner(cold=False))[0] == 0                            # no cap: only the switch drops configuration 2
    assert fake.per_cfg(P7) == [38, 8, 0, 8]


# ------------------------------------------------------------------ choose and the cache file
def test_key_suffix():
    assert T.key_suffix((1, 3, 384, 1248), False, 160 << 10) == "|1x3x384x1248"
    assert T.key_suffix((32, 3, 384, 1248), True, 160 << 10) == "|32x3x384x1248|f16"
    assert T.key_suffix((1, 3, 384, 1248), False, 36 << 10) == "|1x3x384x1248|lds36"
    assert T.key_suffix((1, 3, 8, 8), True, 36 << 10) == "|1x3x8x8|f16|lds36"
    assert T.key_suffix(None, False, 160 << 10) == "|" and T.key_suffix((), False, 160 << 10) == "|"


def conv_cfg(tn, name="conv1{+1 pool}"):
    return tn.conv_cfg(name, (L.ConvDesc * 1)(*descs(7)), 1, SimpleNamespace(ptr=0x40))


def test_choose_precedence_and_replay(install, monkeypatch, tmp_path):
    path = tmp_path / "tune.json"
    key = "conv1{+1 pool}" + SUFFIX
    path.write_text(json.dumps({key: 4}))
    monkeypatch.setenv("FCN_TUNE_CACHE", str(path))
    # the replica's decision comes before the file's, the file's before a search
    fake = install(FakeLib(table(TIMES_ISSUE)))
    tn = tuner(cold=True, tune_from={key: 2})
    assert conv_cfg(tn) == 2 and tn.chosen == {key: 2}
    assert dict(fake.calls) == {"fcn_conv2d_num_configs": 1}         # a replayed decision: no launch, no event, no allocation
    tn = tuner(cold=True, tune_from={"another": 2})
    assert conv_cfg(tn) == 4 and tn.chosen == {key: 4}
    assert dict(fake.calls) == {"fcn_conv2d_num_configs": 2}
    assert json.loads(path.read_text()) == {key: 4}
    # an invalid decision of a replica is passed over
    tn = tuner(cold=True, tune_from={key: 6})
    assert conv_cfg(tn) == 4
    assert not fake.launches


@pytest.mark.parametrize("bad", [6, -1, "3", 2.0, None, [1]])
def test_invalid_cached_configuration_is_searched_again(install, monkeypatch, tmp_path, bad):
    path = tmp_path / "tune.json"
    key = "dgrad:conv2" + SUFFIX
    path.write_text(json.dumps({key: bad, "other|1x1": "01"}))
    monkeypatch.setenv("FCN_TUNE_CACHE", str(path))
    fake = install(FakeLib(table([1.5, 1.0, 2.0]), ncfg=3))
    tn = tuner(cold=False)
    assert conv_cfg(tn, "dgrad:conv2") == 1 and fake.launches
    assert path.read_text() == json.dumps({key: 1, "other|1x1": "01"}, indent=0, sort_keys=True)


def test_cache_file_round_trip(install, monkeypatch, tmp_path):
    path = tmp_path / "tune.json"
    monkeypatch.setenv("FCN_TUNE_CACHE", str(path))      # does not exist yet: an empty cache
    fake = install(FakeLib(table([1.5, 1.0, 2.0]), ncfg=3))
    tn = tuner(cold=False)
    assert conv_cfg(tn, "a+b{+2 pool}{+tail1}") == 1
    chunk = [conv_task("x", 10), conv_task("y", 20)]
    tn.split_level(chunk)
    text = path.read_text()
    assert text == json.dumps({"a+b{+2 pool}{+tail1}" + SUFFIX: 1, "cut|x+y" + SUFFIX: "00"}, indent=0, sort_keys=True)
    fake = install(FakeLib(table([1.5, 1.0, 2.0]), ncfg=3))
    tn2 = tuner(cold=False)
    assert conv_cfg(tn2, "a+b{+2 pool}{+tail1}") == 1 and tn2.split_level(chunk) == [chunk]
    assert tn2.chosen == tn.chosen and not fake.launches and fake.events_made == 0 and not fake.alloc_sizes
    assert path.read_text() == text


def test_unreadable_and_unwritable_cache_file(install, monkeypatch, tmp_path):
    path = tmp_path / "tune.json"
    path.write_text("{ not json")
    monkeypatch.setenv("FCN_TUNE_CACHE", str(path))
    install(FakeLib(table([1.5, 1.0]), ncfg=2))
    assert conv_cfg(tuner(cold=False)) == 1
    assert json.loads(path.read_text()) == {"conv1{+1 pool}" + SUFFIX: 1}
    monkeypatch.setenv("FCN_TUNE_CACHE", str(tmp_path / "no" / "such" / "dir.json"))
    assert conv_cfg(tuner(cold=False)) == 1


# ------------------------------------------------------------------ the cut of a half-float level
def conv_task(name, ident, reads=(), writes=()):
    return ConvTask(SimpleNamespace(name=name), descs(ident)[0], 0.0, 0.0, list(reads), list(writes))


def test_set_partitions():
    for n, parts, subsets in ((2, 2, 3), (3, 5, 7), (4, 15, 15)):
        ps = list(T.set_partitions(n))
        assert len(ps) == parts == len({tuple(p) for p in ps})
        assert len({tuple(i for i in range(n) if p[i] == g) for p in ps for g in set(p)}) == subsets
    assert list(T.set_partitions(3)) == [[0, 0, 0], [0, 0, 1], [0, 1, 0], [0, 1, 1], [0, 1, 2]]


@pytest.mark.parametrize("n,subsets", [(2, 3), (3, 7), (4, 15)])
def test_cut_times_every_subset_once(install, n, subsets):
    # a launch costs 1 ms plus 0.5 ms per convolution in it: one launch for the whole level is cheapest
    fake = install(FakeLib(lambda problem, cfg, nth: 1.0 + 0.5 * (len(problem) - 1), ncfg=1))
    tn = tuner(cold=True)
    chunk = [conv_task("c%d" % i, 10 * (i + 1)) for i in range(n)]
    assert tn.split_level(chunk) == [chunk]
    assert tn.chosen == {"cut|" + "+".join("c%d" % i for i in range(n)) + SUFFIX: "0" * n}
    assert len(fake.launches) == subsets and set(fake.launches.values()) == {8}      # one search each: 1 + 7 cold launches of the one configuration
    assert len(fake.alloc_sizes) == subsets + 1 and len(fake.allocs) == 1           # a workspace per subset, all freed; the eviction buffer lives until release()


def test_cut_returns_the_cheapest_partition(install):
    cost = {(10, 30, 0): 1.0, (20, 0): 0.5}
    fake = install(FakeLib(lambda problem, cfg, nth: cost.get(problem, 2.0 + 0.1 * cfg), ncfg=2))
    tn = tuner(cold=False)
    a, b, c = chunk = [conv_task("a", 10), conv_task("b", 20), conv_task("c", 30)]
    assert tn.split_level(chunk) == [[a, c], [b]]
    assert tn.chosen == {"cut|a+b+c" + SUFFIX: "010"}


def test_cut_keeps_the_first_of_equal_partitions(install):
    fake = install(FakeLib(lambda problem, cfg, nth: 0.25 * (len(problem) - 1), ncfg=1))      # every cut of the level costs the same
    tn = tuner(cold=False)
    chunk = [conv_task("c%d" % i, 10 * (i + 1)) for i in range(4)]
    assert tn.split_level(chunk) == [chunk] and list(tn.chosen.values()) == ["0000"]


@pytest.mark.parametrize("n", [1, 5])
def test_cut_leaves_other_level_sizes_alone(install, n):
    fake = install(FakeLib(table([1.0]), ncfg=1))
    tn = tuner(cold=True)
    chunk = [conv_task("c%d" % i, i) for i in range(n)]
    assert tn.split_level(chunk) == [chunk] and not fake.calls and not tn.chosen


@pytest.mark.parametrize("bad", ["013", "00", "0a0", 1, None])
def test_invalid_cached_cut_is_searched_again(install, monkeypatch, tmp_path, bad):
    path = tmp_path / "tune.json"
    key = "cut|a+b+c" + SUFFIX
    path.write_text(json.dumps({key: bad}))
    monkeypatch.setenv("FCN_TUNE_CACHE", str(path))
    fake = install(FakeLib(lambda problem, cfg, nth: 1.0, ncfg=1))
    tn = tuner(cold=False)
    a, b, c = chunk = [conv_task("a", 10), conv_task("b", 20), conv_task("c", 30)]
    assert tn.split_level(chunk) == [chunk] and fake.launches
    assert json.loads(path.read_text()) == {key: "000"}
    path.write_text(json.dumps({key: "012"}))      # a valid one is replayed
    fake = install(FakeLib(lambda problem, cfg, nth: 1.0, ncfg=1))
    assert tuner(cold=False).split_level(chunk) == [[a], [b], [c]] and not fake.calls


# ------------------------------------------------------------------ levelling, floaters, the move
X, OUT, R3, R5, PL = 0x100, 0x200, 0x300, 0x400, 0x500      # buffers of an inception module: input, concat output, the reduces, the pooled input


def inception():
    """{1x1, 3x3_reduce, 5x5_reduce, pool} then {3x3, 5x5, pool_proj}: the convolutions write their channel slice of the output."""
    x = [(X, 0, 192)]
    pool = OpTask(SimpleNamespace(name="pool"), [], reads=x, writes=[(PL, 0, 192)], pool_desc=L.PoolDesc())
    return [conv_task("1x1", 1, x, [(OUT, 0, 64)]), conv_task("3x3_reduce", 2, x, [(R3, 0, 96)]), conv_task("5x5_reduce", 3, x, [(R5, 0, 16)]), pool,
            conv_task("3x3", 4, [(R3, 0, 96)], [(OUT, 64, 192)]), conv_task("5x5", 5, [(R5, 0, 16)], [(OUT, 192, 224)]),
            conv_task("pool_proj", 6, [(PL, 0, 192)], [(OUT, 224, 256)])]


def test_levels_and_floaters_of_an_inception_module():
    tasks = inception()
    levels = task_levels(tasks)
    assert levels == [0, 0, 0, 0, 1, 1, 1]
    assert [i for i in range(4) if task_floats(tasks, levels, i)] == [0]      # of the first level: the plain 1x1 alone
    assert task_levels(tasks, group_convs=False) == list(range(7))


def test_levels_order_a_write_after_read():
    a = conv_task("a", 1, [(X, 0, 8)], [(OUT, 0, 8)])
    b = conv_task("b", 2, [(R3, 0, 8)], [(X, 4, 12)])           # overwrites part of what a reads
    c = conv_task("c", 3, [(R3, 0, 8)], [(X, 8, 12)])           # not the channels a reads, but some that b writes
    d = conv_task("d", 4, [(R5, 0, 8)], [(OUT, 4, 6)])          # overwrites part of what a wrote
    assert task_levels([a, b, c, d]) == [0, 1, 2, 1]
    assert not task_floats([a, b], [0, 1], 0)


MOVE_KEY = "move|1x1+3x3_reduce+5x5_reduce>3x3+5x5+pool_proj" + SUFFIX


def move_costs(moved_pair_ms):
    """Unmoved: 1.0 + 1.0 ms.  With the 1x1 in the second launch the pair costs moved_pair_ms.  (the first level's pooling rides: 1)"""
    cost = {(1, 2, 3, 1): 1.0, (4, 5, 6, 0): 1.0, (2, 3, 1): 0.4, (4, 5, 6, 1, 0): moved_pair_ms - 0.4}
    return lambda problem, cfg, nth: cost[problem]


@pytest.mark.parametrize("ratio,code", [(0.98, "1"), (0.995, "0")])
def test_move_must_beat_the_margin(install, ratio, code):
    fake = install(FakeLib(move_costs(2.0 * ratio), ncfg=1))
    tn = tuner(cold=True)
    tasks = inception()
    levels = task_levels(tasks)
    tn.move_floaters(tasks, levels)
    assert tn.chosen == {MOVE_KEY: code}
    assert levels == [int(code), 0, 0, 0, 1, 1, 1]
    assert dict(fake.launches) == {(p, 0): 16 for p in ((1, 2, 3, 1), (4, 5, 6, 0), (2, 3, 1), (4, 5, 6, 1, 0))}      # each subset: two searches of 1 + 7


def test_move_margin_switch(install, monkeypatch):
    monkeypatch.setenv("FCN_MOVE_MARGIN", "1.0")
    install(FakeLib(move_costs(2.0 * 0.995), ncfg=1))
    tn = tuner(cold=True)
    tasks = inception()
    tn.move_floaters(tasks, task_levels(tasks))
    assert tn.chosen == {MOVE_KEY: "1"}


def all_floaters():
    x = [(X, 0, 8)]
    return [conv_task("a1", 1, x, [(R3, 0, 8)]), conv_task("a2", 2, x, [(R5, 0, 8)]),
            OpTask(SimpleNamespace(name="p"), [], reads=x, writes=[(PL, 0, 8)]), conv_task("b", 3, [(PL, 0, 8)], [(OUT, 0, 8)])]


def test_move_never_empties_a_level(install, monkeypatch, tmp_path):
    path = tmp_path / "tune.json"
    key = "move|a1+a2>b" + SUFFIX
    path.write_text(json.dumps({key: "11"}))                    # not a valid code here: searched again
    monkeypatch.setenv("FCN_TUNE_CACHE", str(path))
    cost = {(1, 2, 0): 1.0, (3, 0): 1.0, (2, 0): 0.3, (3, 1, 0): 0.3, (1, 0): 0.3, (3, 2, 0): 0.3, (3, 1, 2, 0): 0.01}      # cheapest by far: all three in one launch
    fake = install(FakeLib(lambda problem, cfg, nth: cost[problem], ncfg=1))
    tn = tuner(cold=True)
    tasks = all_floaters()
    levels = task_levels(tasks)
    assert levels == [0, 0, 0, 1]
    tn.move_floaters(tasks, levels)
    assert tn.chosen == {key: "10"} and levels == [1, 0, 0, 1]      # the first of the two equal single moves
    assert ((3, 1, 2, 0), 0) not in fake.launches and json.loads(path.read_text()) == {key: "10"}


def test_move_guards(install):
    fake = install(FakeLib(lambda problem, cfg, nth: 1.0, ncfg=1))
    x = [(X, 0, 8)]
    after = [OpTask(SimpleNamespace(name="p"), [], reads=x, writes=[(PL, 0, 8)]), conv_task("b", 99, [(PL, 0, 8)], [(OUT, 0, 8)])]

    def floaters(n):
        return [conv_task("a%d" % i, i, x, [(0x1000 + i, 0, 8)]) for i in range(n)]

    for tasks in (floaters(1) + after,                      # fewer than two convolutions on the level
                  floaters(4) + after,                      # more than three floaters
                  floaters(9) + after,                      # more than eight convolutions on the level
                  floaters(2),                              # no next level
                  [conv_task("a0", 0, x, [(R3, 0, 8)]), conv_task("a1", 1, x, [(R5, 0, 8)]),      # nothing floats: the next level reads both
                   conv_task("b0", 2, [(R3, 0, 8)], [(OUT, 0, 8)]), conv_task("b1", 3, [(R5, 0, 8)], [(OUT, 8, 16)])]):
        tn = tuner(cold=True)
        levels = task_levels(tasks)
        before = list(levels)
        tn.move_floaters(tasks, levels)
        assert levels == before and not tn.chosen and not fake.calls
    # a next level that would hold more than eight with the floaters
    tasks = floaters(2) + after + [conv_task("b%d" % i, 100 + i, [(PL, 0, 8)], [(OUT, 8 * i + 8, 8 * i + 16)]) for i in range(6)]
    tn = tuner(cold=True)
    tn.move_floaters(tasks, task_levels(tasks))
    assert not tn.chosen and not fake.calls


# ------------------------------------------------------------------ weight gradients
def wgrad_op(fake, name, layers):
    sel = {"cfg": -1}
    op = Op("wgrad", name, lambda st: fake.launch(("wgrad", name), sel["cfg"]))
    op.sel, op.layers = sel, layers
    return op


def test_wgrad_protocol(install, monkeypatch, tmp_path):
    path = tmp_path / "tune.json"
    monkeypatch.setenv("FCN_TUNE_CACHE", str(path))
    times = {"g": [1.0, 1.03, 1.2, 1.035, 1.5], "h": [1.0, 0.5, 0.55, 0.7, 0.51]}
    fake = install(FakeLib(lambda problem, cfg, nth: times[problem[1]][cfg], wgrad_ncfg=5))
    ops = [wgrad_op(fake, "g", ["conv1", "conv2"]), Op("dgrad", "d", None), wgrad_op(fake, "h", ["conv3"])]
    tn = tuner(cold=False)
    tn.wgrad_cfgs(ops)
    assert fake.per_cfg(("wgrad", "g")) == [27, 27, 7, 27, 7, 0]      # 2 + 5, then 4 x 5 for the three within 4 %
    assert fake.per_cfg(("wgrad", "h")) == [7, 27, 7, 7, 27, 0]       # (0.55 is outside)
    assert [op.name for op in ops] == ["g [cfg0]", "d", "h [cfg1]"] and [ops[0].sel["cfg"], ops[2].sel["cfg"]] == [0, 1]
    want = {"wgrad:conv1+conv2" + SUFFIX: 0, "wgrad:conv3" + SUFFIX: 1}
    assert tn.chosen == want and path.read_text() == json.dumps(want, indent=0, sort_keys=True)
    # replay
    fake = install(FakeLib(lambda problem, cfg, nth: 1.0, wgrad_ncfg=5))
    ops = [wgrad_op(fake, "g", ["conv1", "conv2"]), wgrad_op(fake, "h", ["conv3"])]
    tn = tuner(cold=False)
    tn.wgrad_cfgs(ops)
    assert [op.name for op in ops] == ["g [cfg0]", "h [cfg1]"] and tn.chosen == want
    assert dict(fake.calls) == {"fcn_conv2d_wgrad_num_configs": 1} and not fake.launches


def test_wgrad_single_configuration(install):
    fake = install(FakeLib(lambda problem, cfg, nth: 1.0, wgrad_ncfg=1))
    ops = [wgrad_op(fake, "g", ["conv1"])]
    tuner(cold=False).wgrad_cfgs(ops)
    assert fake.per_cfg(("wgrad", "g"))[0] == 7 and ops[0].name == "g [cfg0]"


# ------------------------------------------------------------------ release
def test_release(install):
    fake = install(FakeLib(table(TIMES_ISSUE)))
    tn = tuner(cold=True)
    one_problem(tn)
    tn.split_level([conv_task("x", 10), conv_task("y", 20)])
    assert fake.events_made == 2 and len(fake.events_live) == 2 and list(fake.allocs.values()) == [64 << 20]
    tn.release()
    assert not fake.events_live and not fake.allocs and fake.calls["fcn_event_destroy"] == 2
    calls = dict(fake.calls)
    tn.release()
    assert dict(fake.calls) == calls
    # a tuner that timed nothing has nothing to release
    tn = tuner(cold=True, tune_from={"conv1{+1 pool}" + SUFFIX: 3})
    conv_cfg(tn)
    calls = dict(fake.calls)
    tn.release()
    assert dict(fake.calls) == calls
