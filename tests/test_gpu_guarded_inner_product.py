"""Guard-banded, poisoned-buffer parity of the InnerProduct kernels against the float64 reference (tests/ref_ip64.py), -m gpu.

Every operand lies in a buffer with 256 KiB red zones (tests/gpu_util.py); rows are padded with NaN poison behind their K elements
and y / dY are channel slices of wider pixels whose other channels hold poison, so a read outside a row or a write outside the slice
shows.  float32 results are held to ref64.dot_bound_rms against float64, half-float ones to the float64 product of the ROUNDED
operands plus one final rounding; every case is launched twice and must give identical bits."""
import numpy as np
import pytest

import ref64
import ref_ip64 as R
from fcn_object_detector_amd import lib as L
from gpu_util import Guards, poison_free, poisoned, slice_untouched

pytestmark = pytest.mark.gpu
RELU, ACCUM, OUT_F32, NT = 1, 4, 8, 256


@pytest.fixture
def g(gpu):
    with Guards() as guards:
        yield guards


def rows(a, rstride, dtype=np.float32):
    """(M, K) -> (M, rstride) with NaN behind the K elements of every row"""
    out = poisoned((a.shape[0], rstride), dtype=dtype)
    out[:, :a.shape[1]] = a
    return out


def in_slice(a, cstride, coffset, dtype=np.float32):
    out = poisoned((a.shape[0], cstride), dtype=dtype)
    out[:, coffset:coffset + a.shape[1]] = a
    return out


def workspace(g, M, K, N):
    n = L.load().fcn_inner_product_workspace_bytes(M, K, N)
    return g.put(int(n), name="workspace").ptr if n else None


def twice(call, read):
    call()
    a = read()
    call()
    b = read()
    assert a.tobytes() == b.tobytes(), "two launches differ"
    return a


# M, K, N, x_rstride - K, y_cstride, y_coffset, flags
FWD = [
    (1, 256, 4, 0, 4, 0, 0),
    (3, 1000, 10, 8, 16, 4, RELU),               # K is not a multiple of a wave's 256-element step; y inside a wider pixel
    (8, 9216, 1000, 0, 1000, 0, 0),              # CaffeNet-like, the K slices of a 1000-output layer
    (9, 256, 4096, 16, 4096, 0, RELU | NT),
    (32, 1000, 10, 0, 24, 8, NT),
    (1, 9216, 4096, 0, 4096, 0, RELU),           # fc6 of CaffeNet at batch 1
    (10, 4096, 4, 0, 8, 4, 0),                   # GOTURN's fc8-shapes
    (2, 18432, 10, 0, 16, 0, 0),                 # two towers' pool5
    (5, 4096, 1001, 0, 1008, 0, 0),              # rows of w past the last whole group of four
]


@pytest.mark.parametrize("case", FWD)
def test_forward_f32(g, case):
    M, K, N, pad, ycs, yco, flags = case
    rng = np.random.default_rng(FWD.index(case))
    x, w, b = (rng.standard_normal(s).astype(np.float32) for s in ((M, K), (N, K), (N,)))
    xd, wd, bd = g.put(rows(x, K + pad), name="x"), g.put(w, at_end=True, name="w"), g.put(b, name="bias")
    yd = g.put(poisoned((M, ycs)), name="y")
    ws = workspace(g, M, K, N)
    full = twice(lambda: L.call("fcn_inner_product_fwd_f32", xd.ptr, K + pad, wd.ptr, bd.ptr, yd.ptr, ycs, yco, M, K, N, flags, ws, None),
                 lambda: yd.read((M, ycs)))
    y = full[:, yco:yco + N]
    assert poison_free(y) and slice_untouched(full, yco, N)
    want = R.forward(x, w, b, relu=bool(flags & RELU))
    assert np.all(np.abs(y - want) <= ref64.dot_bound_rms(K, R.magnitude(x, w, b)))
    assert np.abs(y - want).max() <= 1e-4 * np.abs(want).max()
    L.call("fcn_inner_product_fwd_f32", xd.ptr, K + pad, wd.ptr, None, yd.ptr, ycs, yco, M, K, N, flags & RELU, ws, None)      # bias_term: false
    y0 = yd.read((M, ycs))[:, yco:yco + N]
    assert np.all(np.abs(y0 - R.forward(x, w, None, relu=bool(flags & RELU))) <= ref64.dot_bound_rms(K, R.magnitude(x, w)))


@pytest.mark.parametrize("out_f32", [False, True], ids=["y16", "y32"])
@pytest.mark.parametrize("case", FWD)
def test_forward_f16(g, case, out_f32):
    M, K, N, pad, ycs, yco, flags = case
    pad, ycs, yco = 2 * pad, (ycs if out_f32 else 2 * ycs), (yco if out_f32 else 2 * yco)
    rng = np.random.default_rng(100 + FWD.index(case))
    x, w = (rng.standard_normal(s).astype(np.float16) for s in ((M, K), (N, K)))
    w = (w / np.float16(8)).astype(np.float16)
    b = rng.standard_normal(N).astype(np.float32)
    ydt = np.float32 if out_f32 else np.float16
    xd, wd, bd = g.put(rows(x, K + pad, np.float16), name="x"), g.put(w, at_end=True, name="w"), g.put(b, name="bias")
    yd = g.put(poisoned((M, ycs), dtype=ydt), name="y")
    ws = workspace(g, M, K, N)
    fl = flags | (OUT_F32 if out_f32 else 0)
    full = twice(lambda: L.call("fcn_inner_product_fwd_f16", xd.ptr, K + pad, wd.ptr, bd.ptr, yd.ptr, ycs, yco, M, K, N, fl, ws, None),
                 lambda: yd.read((M, ycs), ydt))
    y = full[:, yco:yco + N]
    assert poison_free(y) and slice_untouched(full, yco, N)
    want = R.forward(x, w, b, relu=bool(flags & RELU))
    tol = ref64.dot_bound_rms(K, R.magnitude(x, w, b)) + (0 if out_f32 else ref64.U16 * np.abs(want) + 2.0 ** -24)
    assert np.all(np.abs(y.astype(np.float64) - want) <= tol)


# M, K, N, dy_cstride, dy_coffset, dx_rstride - K
BWD = [
    (1, 256, 4, 4, 0, 0),
    (3, 1000, 10, 16, 4, 8),
    (8, 9216, 1000, 1000, 0, 0),
    (9, 256, 4096, 4096, 0, 4),
    (32, 1000, 10, 24, 8, 0),
    (8, 18432, 64, 64, 0, 0),
    (32, 4096, 4096, 4096, 0, 0),
]


@pytest.mark.parametrize("case", BWD)
def test_backward_data(g, case):
    M, K, N, dcs, dco, pad = case
    rng = np.random.default_rng(200 + BWD.index(case))
    dy, w, base = (rng.standard_normal(s).astype(np.float32) for s in ((M, N), (N, K), (M, K)))
    dyd, wd = g.put(in_slice(dy, dcs, dco), at_end=True, name="dy"), g.put(w, at_end=True, name="w")
    dxd = g.put(poisoned((M, K + pad)), name="dx")
    ws = workspace(g, M, K, N)
    full = twice(lambda: L.call("fcn_inner_product_bwd_data_f32", dyd.ptr, dcs, dco, wd.ptr, dxd.ptr, K + pad, M, K, N, 0, ws, None),
                 lambda: dxd.read((M, K + pad)))
    assert poison_free(full[:, :K]) and slice_untouched(full, 0, K)
    bound = ref64.dot_bound_rms(N, np.abs(dy).astype(np.float64) @ np.abs(w).astype(np.float64))
    assert np.all(np.abs(full[:, :K] - R.bwd_data(dy, w)) <= bound)
    dxa = g.put(rows(base, K + pad), name="dx (accumulate)")
    L.call("fcn_inner_product_bwd_data_f32", dyd.ptr, dcs, dco, wd.ptr, dxa.ptr, K + pad, M, K, N, ACCUM, ws, None)
    acc = dxa.read((M, K + pad))
    assert slice_untouched(acc, 0, K)
    assert np.all(np.abs(acc[:, :K] - R.bwd_data(dy, w, dx=base)) <= bound + 2.0 ** -23 * np.abs(R.bwd_data(dy, w, dx=base)))
    assert np.array_equal(acc[:, :K], (full[:, :K] + base).astype(np.float32))      # one correctly rounded add on the plain result


@pytest.mark.parametrize("with_db", [True, False], ids=["db", "nodb"])
@pytest.mark.parametrize("case", BWD)
def test_backward_weights(g, case, with_db):
    M, K, N, dcs, dco, pad = case
    rng = np.random.default_rng(300 + BWD.index(case))
    x, dy = (rng.standard_normal(s).astype(np.float32) for s in ((M, K), (M, N)))
    xd, dyd = g.put(rows(x, K + pad), name="x"), g.put(in_slice(dy, dcs, dco), at_end=True, name="dy")
    dwd, dbd = g.put(poisoned((N, K)), at_end=True, name="dw"), g.put(poisoned((N,)), name="db")
    db_ptr = dbd.ptr if with_db else None
    call = lambda acc: L.call("fcn_inner_product_bwd_weights_f32", xd.ptr, K + pad, dyd.ptr, dcs, dco, dwd.ptr, db_ptr, M, K, N, acc, None)
    dw = twice(lambda: call(0), lambda: dwd.read((N, K)))
    gw, gb = R.bwd_weights(x, dy)
    bound = ref64.dot_bound_rms(M, np.abs(dy).T.astype(np.float64) @ np.abs(x).astype(np.float64))
    assert poison_free(dw) and np.all(np.abs(dw - gw) <= bound)
    if with_db:
        db = dbd.read((N,))
        assert np.all(np.abs(db - gb) <= ref64.dot_bound_rms(M, np.abs(dy).sum(axis=0)))
    else:
        assert dbd.unchanged()
    call(1)                                                  # iter_size: a second micro-batch adds
    dw2 = dwd.read((N, K))
    assert np.all(np.abs(dw2 - 2 * gw) <= 2 * bound + 2.0 ** -23 * np.abs(2 * gw))
    if with_db:
        assert np.array_equal(dbd.read((N,)), (db + db).astype(np.float32))


def test_refusals_leave_the_buffers_alone(g):
    M, K, N = 2, 512, 40
    xd, wd, yd = g.put(poisoned((M, K)), name="x"), g.put(poisoned((N, K)), name="w"), g.put(poisoned((M, 64)), name="y")
    lib = L.load()
    assert lib.fcn_inner_product_workspace_bytes(M, K, N) >= lib.fcn_inner_product_fwd_workspace_bytes(M, K, N, 4) >= 0
    for fn in (lib.fcn_inner_product_fwd_f32, lib.fcn_inner_product_fwd_f16):
        assert fn(None, K, wd.ptr, None, yd.ptr, 64, 0, M, K, N, 0, None, None) == 1
        assert fn(xd.ptr + 4, K, wd.ptr, None, yd.ptr, 64, 0, M, K, N, 0, None, None) == 2
        assert fn(xd.ptr, K, wd.ptr, None, yd.ptr, 64, 0, 33, K, N, 0, None, None) == 3
    assert lib.fcn_inner_product_bwd_data_f32(yd.ptr, 64, 32, wd.ptr, xd.ptr, K, M, K, N, 0, None, None) == 1
    assert lib.fcn_inner_product_bwd_weights_f32(xd.ptr, K, yd.ptr, 64, 0, wd.ptr, None, M, K, N, 2, None) == 1
    L.call("fcn_device_sync")
    assert xd.unchanged() and wd.unchanged() and yd.unchanged()
