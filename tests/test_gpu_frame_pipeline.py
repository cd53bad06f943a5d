"""Frame pipelines on replica streams (run with -m gpu): every replica of a ForwardPipeline takes its stream from
fcn_stream_create_replica (a hardware queue of its own under the runtime's default queue limit).  Results are those of
Engine.forward() on a lone engine (plain stream) with the same tile plan, bit for bit and in input order."""
import ctypes as C

import numpy as np
import pytest

from fcn_object_detector_amd import lib as L, models, proto
from fcn_object_detector_amd.engine import DeviceBuffer, Engine, ForwardPipeline
from fcn_object_detector_amd.netspec import NetSpec, fill_params

pytestmark = pytest.mark.gpu
H, W, CLASSES, DEPTH, FRAMES = 96, 128, 2, 4, 12
HEADS = ("coverage", "bboxes")


@pytest.fixture(scope="module")
def net(gpu):
    """The 96x128 deploy net, 12 distinct frames and what a lone engine's forward() gives for each (computed once, never written)."""
    msg = proto.parse_text(models.googlenet_detectnet_deploy(1, H, W, CLASSES))
    spec = NetSpec(msg, "TEST")
    spec.infer()
    params = fill_params(spec, seed=1234)
    rng = np.random.default_rng(21)
    frames = [rng.random((1, 3, H, W), dtype=np.float32) for _ in range(FRAMES)]
    lone = Engine(NetSpec(msg, "TEST"), params=params, device=0, autotune=False)
    assert lone.replica is None and not lone.stream_prioritized      # lone engines keep plain streams
    want = []
    for f in frames:
        lone.host_array("data")[...] = f
        want.append({k: v.copy() for k, v in lone.forward().items()})
    lone.close()
    for w in want:
        for v in w.values():
            v.setflags(write=False)
    assert not np.array_equal(want[0]["coverage"], want[1]["coverage"])
    return msg, params, frames, want


def make_pipe(net, depth=DEPTH):
    msg, params, _, _ = net
    return ForwardPipeline(lambda: NetSpec(msg, "TEST"), params=params, device=0, depth=depth, autotune=False)


def same(got, want):
    return all(np.array_equal(got[k], want[k]) for k in HEADS)


def test_map_equals_lone_forward_in_input_order(net):
    _, _, frames, want = net
    pipe = make_pipe(net)
    assert [e.replica for e in pipe.engines] == [0, 1, 2, 3] and all(e.stream_prioritized for e in pipe.engines)
    got = pipe.map([{"data": f} for f in frames])
    assert len(got) == FRAMES
    for i, (g, w) in enumerate(zip(got, want)):
        assert same(g, w), i
    assert len({e.stream for e in pipe.engines}) == DEPTH
    pipe.close()


def test_run_io_then_read_blob_on_the_last_replica(net):
    """What bench.py --dump-outputs relies on: after run_io the replica that ran the last frame holds that frame's outputs in its
    host arrays, read_blob() returns them without another download, and an inner blob is still fetched on demand."""
    _, _, frames, want = net
    pipe = make_pipe(net)
    for i, e in enumerate(pipe.engines):
        e.host_array("data")[...] = frames[i]
    iters = 10
    assert pipe.run_io(iters, DEPTH) > 0
    last = pipe.engines[(iters - 1) % DEPTH]
    w = want[(iters - 1) % DEPTH]
    assert all(last.blobs[k].host_valid for k in HEADS) and last.blobs["data"].host_valid
    inner = "inception_5b/output"
    assert not last.blobs[inner].host_valid
    for k in HEADS:
        assert np.array_equal(last.read_blob(k), w[k])
    a = last.read_blob(inner)
    assert last.blobs[inner].host_valid and np.isfinite(a).all() and np.abs(a).max() > 0
    last.forward_begin()
    last.forward_end()
    assert not last.blobs[inner].host_valid and same({k: last.read_blob(k) for k in HEADS}, w)
    pipe.close()


def test_a_fifth_submit_without_a_collect_raises(net):
    _, _, frames, want = net
    pipe = make_pipe(net)
    for f in frames[:DEPTH]:
        pipe.submit({"data": f})
    with pytest.raises(RuntimeError):
        pipe.submit({"data": frames[DEPTH]})
    for i in range(DEPTH):                                   # the refused frame disturbed nothing; collection is in order
        assert same(pipe.collect(), want[i]), i
    with pytest.raises(RuntimeError):
        pipe.collect()
    pipe.close()


def test_close_then_a_second_pipeline(net):
    _, _, frames, want = net
    pipe = make_pipe(net)
    assert same(pipe.map([{"data": frames[0]}])[0], want[0])
    pipe.close()
    assert all(e.stream == 0 for e in pipe.engines)
    pipe.close()                                                    # closing twice is harmless
    again = make_pipe(net)
    got = again.map([{"data": f} for f in frames[:6]])
    assert all(same(g, w) for g, w in zip(got, want))
    again.close()


def test_no_graph_gives_equal_results(net, monkeypatch):
    _, _, frames, want = net
    monkeypatch.setenv("FCN_NO_GRAPH", "1")
    pipe = make_pipe(net)
    got = pipe.map([{"data": f} for f in frames[:6]])
    assert all(same(g, w) for g, w in zip(got, want))
    assert all(e.graph_io is None for e in pipe.engines)
    pipe.close()


def test_replica_streams_are_distinct_and_usable(gpu):
    lib = L.load()
    n = 1000
    x = np.linspace(-1, 1, n).astype(np.float32)
    streams = []
    kinds = []
    for index in (0, 1, 2, 3, -1, L.REPLICA_STREAMS):      # the last two: out of range -> the fallback, a plain stream
        s, yes = C.c_void_p(), C.c_int(-1)
        L.call("fcn_stream_create_replica", C.byref(s), index)
        assert s.value
        L.call("fcn_stream_is_prioritized", s, C.byref(yes))
        streams.append(int(s.value))
        kinds.append(yes.value)
    assert len(set(streams)) == len(streams)
    # an MI355X has stream priorities: a replica stream that comes back plain means the runtime refused, and four in flight alias again
    assert kinds == [1, 1, 1, 1, 0, 0]
    plain, yes = C.c_void_p(), C.c_int(-1)
    L.call("fcn_stream_create", C.byref(plain))
    L.call("fcn_stream_is_prioritized", plain, C.byref(yes))
    assert yes.value == 0
    L.call("fcn_stream_destroy", plain)
    bufs, outs = [], []
    for k, s in enumerate(streams):      # a kernel on each, all enqueued before any is waited for
        d = DeviceBuffer(2 * n * 4)
        h = np.ascontiguousarray(x * (k + 1))
        o = np.zeros(n, np.float32)
        L.call("fcn_memcpy_h2d_async", d.ptr, h.ctypes.data, n * 4, s)
        L.check(lib.fcn_relu_fwd_f32(d.ptr, d.ptr + n * 4, n, 0.0, s))
        L.call("fcn_memcpy_d2h_async", o.ctypes.data, d.ptr + n * 4, n * 4, s)
        bufs.append((d, h))
        outs.append(o)
    for k, s in enumerate(streams):
        L.call("fcn_stream_sync", s)
        assert np.array_equal(outs[k], np.maximum(bufs[k][1], 0)), k
    for s in streams:
        L.call("fcn_stream_destroy", s)
    for d, _ in bufs:
        d.free()
