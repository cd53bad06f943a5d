"""The one engine stub of the plan tests: Engine / TrainEngine / BackwardPlanner methods run without a GPU.

engine_factory(monkeypatch, ...) returns make(text, phase, ...): an engine made by blank() - `__new__` + `_init_state`, the state
Engine.__init__ itself starts from, so no list of attributes here - with DeviceBuffer replaced by a counter of addresses and the library by one that records
every call and returns 0 (size queries: 64).  Its buffers, parameters and forward tasks are planned; a TRAIN engine's backward plan too,
and adopted as TrainEngine._build_backward adopts it.  What the stub adds to the engine: .fake (the FakeLib), .copies / .copied (what was
'uploaded': in order, and by address), .tasks and .plan.

Each plan-test file keeps a `stub` fixture of its own that calls engine_factory with the NetSpec keywords that file plans under (none: a
bare NetSpec, which refuses the newer layers by name; public=True: NetSpec.public's rule)."""
import ctypes as C

from fcn_object_detector_amd import backward as BW
from fcn_object_detector_amd import engine as E
from fcn_object_detector_amd import lib as L
from fcn_object_detector_amd import proto
from fcn_object_detector_amd import train as T
from fcn_object_detector_amd.netspec import NetSpec, fill_params


class FakeBuffer:
    next_ptr = 1 << 20

    def __init__(self, nbytes, zero=True):
        self.ptr, self.nbytes = FakeBuffer.next_ptr, int(nbytes)
        FakeBuffer.next_ptr += (int(nbytes) + 4095) // 4096 * 4096 + 4096

    def free(self):
        pass


class FakeLib:
    """Every entry point exists, records (name, args) and returns 0 - 64 where the name says it is a size query."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def fn(*a):
            self.calls.append((name, a))
            return 64 if name.endswith("_bytes") else 0
        return fn

    def names(self):
        return [name for name, _a in self.calls]

    @property
    def args(self):
        """Entry point -> the arguments of its last call."""
        return dict(self.calls)


def blank(cls, spec, **state):
    """An engine of class cls with the state of _init_state and nothing else: no device, no buffer, no plan."""
    e = cls.__new__(cls)
    e._init_state(spec, **state)
    return e


def engine_factory(monkeypatch, public=False, f16=False, backward=True, **spec_defaults):
    """make(text, phase="TEST", f16=f16, backward=backward, fuse=True, **spec_kw) -> the planned stub engine.  The NetSpec gets spec_defaults
    (over NetSpec.public_features(phase) if public) and then spec_kw."""
    lib, copies, copied = FakeLib(), [], {}

    def call(name, *a):
        lib.calls.append((name, a))
        if name == "fcn_memcpy_h2d_async":
            copies.append((int(a[0]), C.string_at(a[1], a[2])))
            copied[int(a[0])] = copies[-1][1]
    for mod in (E, BW, T):
        monkeypatch.setattr(mod, "DeviceBuffer", FakeBuffer)
    monkeypatch.setattr(L, "call", call)
    monkeypatch.setattr(L, "load", lambda: lib)

    def make(text, phase="TEST", f16=f16, backward=backward, fuse=True, **spec_kw):
        FakeBuffer.next_ptr = 1 << 20
        spec = NetSpec(proto.parse_text(text), phase, **{**(NetSpec.public_features(phase) if public else {}), **spec_defaults, **spec_kw})
        e = blank(T.TrainEngine if phase == "TRAIN" else E.Engine, spec, dtype="f16" if f16 else "f32", fuse=fuse, autotune=False)
        e.fake, e.copies, e.copied = lib, copies, copied
        e._plan_buffers()
        e._alloc_params(fill_params(spec, seed=1))
        if phase == "TRAIN":
            e.grad_flat = FakeBuffer(4 * e.param_count)
        e.tasks = e._collect_tasks()
        if phase == "TRAIN" and backward:
            e.plan = BW.BackwardPlanner(e)
            e.plan.run()
            e._adopt_backward(e.plan)
        if e._bn_ws_bytes:
            e._bn_ws = FakeBuffer(e._bn_ws_bytes)      # (as Engine._build_ops, for a test that runs a BatchNorm op)
        return e
    return make
