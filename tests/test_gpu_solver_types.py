"""The solver types, clip_gradients and iter_size on the DetectNet training net at reduced size, on the GPU (-m gpu): every update is
held to the float64 restatement (tests/ref_solver64.py) applied to the gradients the engine itself returns, accumulation to the
equivalent larger batch, and `caffe train` runs, snapshots and resumes a solver file that uses all of it."""
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import ref_solver64 as S
from conftest import rel_err
from fcn_object_detector_amd import models, proto
from fcn_object_detector_amd.netspec import NetSpec, fill_params
from fcn_object_detector_amd.train import SolverParams, TrainEngine
from test_gpu_train import make_batch

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAFFE = os.path.join(REPO, "fcn_object_detector_amd", "build", "tools", "caffe")
PYDIR = os.path.join(REPO, "fcn_object_detector_amd", "python")
U32 = 2.0 ** -24
H, W = 96, 128

TYPES = {
    "NESTEROV": dict(base_lr=1e-3, momentum=0.9, weight_decay=1e-4),
    "ADAGRAD": dict(base_lr=1e-4, weight_decay=1e-5, regularization_type="L1"),
    "RMSPROP": dict(base_lr=1e-4, rms_decay=0.98, weight_decay=1e-4),
    "ADADELTA": dict(base_lr=0.1, momentum=0.95, delta=1e-6, weight_decay=1e-4),
}


def engine(n, **solver):
    msg = proto.parse_text(models.googlenet_detectnet_train("m", "L", "unused", num_classes=1))
    shapes = {k: v.shape for k, v in make_batch(np.random.default_rng(0), n, H, W).items()}
    spec = NetSpec(msg, "TRAIN")
    spec.infer(shapes)
    params = fill_params(spec, seed=1234)
    sp = SolverParams(**solver)
    return TrainEngine(NetSpec(msg, "TRAIN"), shapes, params=params, device=0, solver=sp, autotune=False), spec, sp


def fill(eng, batch):
    for k, v in batch.items():
        eng.host_array(k)[...] = v


def blobs(spec, per_layer):
    """[(layer, index, array, lr_mult, decay_mult)] in the order of the solver's history"""
    out = []
    for l in spec.param_layers():
        for i, a in enumerate(per_layer[l.name]):
            out.append((l.name, i, a, l.lr_mult[i] if i < len(l.lr_mult) else 1.0, l.decay_mult[i] if i < len(l.decay_mult) else 1.0))
    return out


def reference_step(spec, sp, it, w0, g, hist, grad_scale=1.0, clip=1.0):
    """The float64 update of every blob, [(layer, index, (w, h1, h2), (dw, dh1, dh2))]: the second triple is what the float32 rounding
    of g' = g * grad_scale * clip + regularisation (2 u of its two terms; they may cancel) does to each output, found by evaluating the
    rule at g' +- that."""
    ws, gs = blobs(spec, w0), blobs(spec, g)
    n = len(ws)
    f = S.f32
    rate = f(S.rate(sp.lr_policy, it, sp.base_lr, sp.gamma, sp.power, sp.stepsize, sp.stepvalue, sp.max_iter))
    hyp = dict(momentum=f(sp.momentum), momentum2=f(sp.momentum2), rms_decay=f(sp.rms_decay), delta=f(sp.delta), t=it + 1)
    out = []
    for k, ((layer, i, w, lr_mult, decay_mult), (_, _, gr, _, _)) in enumerate(zip(ws, gs)):
        w, gr, h1 = (np.asarray(a, np.float64) for a in (w, gr, hist[k]))
        h2 = np.asarray(hist[n + k], np.float64) if sp.histories == 2 else None
        if lr_mult == 0:
            out.append((layer, i, (w, h1, h2), (0.0, 0.0, 0.0)))
            continue
        term_g = gr * grad_scale * clip
        term_r = f(sp.weight_decay) * decay_mult * (w if sp.regularization_type == "L2" else np.sign(w))
        gg, eg = term_g + term_r, 2 * U32 * (np.abs(term_g) + np.abs(term_r))
        assert np.array_equal(gg, S.effective_gradient(w, gr, f(sp.weight_decay), decay_mult, grad_scale, clip, sp.regularization_type))
        ref, lo, hi = (S.update_from_gradient(sp.kind, w, x, h1, h2, rate, lr_mult, **hyp) for x in (gg, gg - eg, gg + eg))
        prop = tuple(np.maximum(np.abs(a - c), np.abs(b - c)) if c is not None else 0.0 for a, b, c in zip(lo, hi, ref))
        out.append((layer, i, ref, prop))
    return out


def check_step(spec, sp, it, w0, g, hist, w1, hist1, grad_scale=1.0, clip=1.0, what=""):
    ref = reference_step(spec, sp, it, w0, g, hist, grad_scale, clip)
    n, moved = len(ref), 0.0
    for k, (layer, i, (w64, h64, h2_64), (pw, ph, ph2)) in enumerate(ref):
        old, got = np.asarray(w0[layer][i], np.float64), np.asarray(w1[layer][i], np.float64)
        delta = np.abs(w64 - old)
        allow = pw + 8 * U32 * (np.abs(old) + delta) + 1e-5 * delta + 1e-37
        bad = np.abs(got - w64) / allow
        assert bad.max() <= 1.0, "%s %s[%d] iteration %d: weights off by %.3g of the allowance" % (what, layer, i, it, bad.max())
        moved = max(moved, float(delta.max()))
        for got_h, want_h, old_h, p in ((hist1[k], h64, hist[k], ph),) + (((hist1[n + k], h2_64, hist[n + k], ph2),) if h2_64 is not None else ()):
            allow = p + 8 * U32 * (np.abs(want_h) + np.abs(old_h)) + 2e-5 * np.abs(want_h - old_h) + 1e-37
            bad = np.abs(np.asarray(got_h, np.float64) - want_h) / allow
            assert bad.max() <= 1.0, "%s %s[%d] iteration %d: history off by %.3g of the allowance" % (what, layer, i, it, bad.max())
    assert moved > 0, "nothing moved"


@pytest.mark.parametrize("kind", sorted(TYPES))
def test_three_steps_equal_the_float64_rule_on_the_engines_own_gradients(gpu, kind):
    eng, spec, sp = engine(2, solver_type=kind, lr_policy="multistep", stepvalue=[1, 2], gamma=0.5, **TYPES[kind])
    assert eng.solver.kind == kind and (eng.hist2 is not None) == (kind == "ADADELTA")
    for it in range(3):
        fill(eng, make_batch(np.random.default_rng(50 + it), 2, H, W))
        w0, hist = eng.download_params(), eng.download_history()
        out = eng.step(seed=100 + it)
        assert np.isfinite(out["total_loss"]) and eng.iter == it + 1
        check_step(spec, sp, it, w0, eng.download_grads(), hist, eng.download_params(), eng.download_history(), what=kind)
    eng.close()


def test_clip_gradients_scales_the_update_by_the_reference_factor(gpu):
    solver = dict(solver_type="NESTEROV", base_lr=1e-3, momentum=0.9, weight_decay=1e-6)
    batch = make_batch(np.random.default_rng(61), 2, H, W)
    free, spec, _ = engine(2, **solver)
    fill(free, batch)
    free.step(seed=3)
    norm = np.sqrt(sum(float(np.sum(np.asarray(a, np.float64) ** 2)) for v in free.download_grads().values() for a in v))
    assert free.read_clip()[0] == 1.0 and norm > 0
    eng, spec, sp = engine(2, clip_gradients=0.3 * norm, **solver)      # a threshold that bites: the factor is about 0.3
    w0, hist = eng.download_params(), eng.download_history()
    fill(eng, batch)
    eng.step(seed=3)
    g = eng.download_grads()
    sumsq = sum(float(np.sum(np.asarray(a, np.float64) ** 2)) for v in g.values() for a in v)
    want = S.clip_factor(sumsq, S.f32(0.3 * norm))
    clip, dev_sumsq = eng.read_clip()
    assert 0.29 < want < 0.31
    assert abs(dev_sumsq - sumsq) <= 1e-6 * sumsq and abs(clip - want) <= 4 * U32 * want
    check_step(spec, sp, 0, w0, g, hist, eng.download_params(), eng.download_history(), clip=clip, what="clipped")
    # ... and the unclipped engine moved 1 / clip times as far (the tiny weight decay aside: compare the largest momentum history)
    ha, hb = eng.download_history(), free.download_history()
    big = int(np.argmax([np.abs(h).max() for h in hb]))
    assert rel_err(ha[big] / want, hb[big]) < 1e-2
    with pytest.raises(AssertionError):      # (the check has teeth: without the factor the same comparison fails)
        check_step(spec, sp, 0, w0, g, hist, eng.download_params(), eng.download_history(), clip=1.0)
    eng.close()
    free.close()


def test_iter_size_2_on_batch_4_equals_batch_8(gpu):
    """L1Loss and EuclideanLoss divide by the batch, so each batch-4 pass yields TWICE its share of the batch-8 gradient: the accumulated
    buffer is 2 x the batch-8 gradient, the 1 / iter_size normalisation brings the update back to batch 8's (expected factor 1), and the
    mean of the two pass losses is the batch-8 loss.  A single batch-4 step - what iter_size used to do, with half the gradient - differs."""
    solver = dict(base_lr=1e-3, momentum=0.9, weight_decay=1e-6)
    big = make_batch(np.random.default_rng(77), 8, H, W)
    halves = [{k: v[4 * j:4 * j + 4] for k, v in big.items()} for j in range(2)]
    e8, spec, _ = engine(8, **solver)
    e42, _, _ = engine(4, iter_size=2, **solver)
    e4, _, _ = engine(4, **solver)
    w0 = e8.download_params()
    drop = int(np.prod(e42.blobs["pool5/drop_s1"].shape))

    def feed(j):
        fill(e42, halves[j])
        e42.dropout_index_offset = j * drop      # sample 4 j + i draws the dropout mask it has as sample of the batch of 8

    fill(e8, big)
    out8 = e8.step(seed=5)
    out42 = e42.step(seed=5, feed=feed)
    fill(e4, halves[0])
    e4.step(seed=5)
    assert e42.iter == 1 and e8.iter == 1
    assert abs(out42["total_loss"] - out8["total_loss"]) < 1e-4 * abs(out8["total_loss"])
    g8, g42 = e8.download_grads(), e42.download_grads()
    w8, w42, w4 = e8.download_params(), e42.download_params(), e4.download_params()
    differs = 0
    for name in ("conv1/7x7_s2", "inception_3a/3x3", "inception_4c/1x1", "inception_5b/5x5", "bbox/regressor", "cvg/classifier"):
        assert rel_err(g42[name][0], 2.0 * g8[name][0]) < 2e-3, name      # summation order (and a ReLU mask bit here and there)
        d8, d42, d4 = (w[name][0].astype(np.float64) - w0[name][0] for w in (w8, w42, w4))
        assert rel_err(d42, d8) < 2e-3, name
        differs += rel_err(d4, d8) > 5e-2
    assert differs >= 5
    for e in (e8, e42, e4):
        e.close()


def test_iter_size_passes_are_separate_calls_and_iter_moves_once(gpu):
    eng, spec, sp = engine(2, solver_type="RMSPROP", base_lr=1e-4, iter_size=3)
    losses, raw = [], []
    for j in range(3):
        fill(eng, make_batch(np.random.default_rng(90 + j), 2, H, W))
        eng.step_begin(seed=j)
        assert eng.iter == 0
        losses.append(eng.step_end())
        raw.append(float(eng.loss_host["loss_bbox"][0]))      # the pass's own value
    assert eng.iter == 1 and len(set(raw)) == 3
    assert losses[2]["loss_bbox"] == pytest.approx(np.mean(raw), rel=1e-12) and losses[0]["loss_bbox"] == raw[0]
    eng.close()


# ---- through the Solver front end and the tool ----------------------------------------------------------------------------------
def write_job(tmp_path, extra, max_iter=4, snapshot=2):
    net = tmp_path / "train_val.prototxt"
    net.write_text(models.googlenet_detectnet_train("data_argumentation_layer", "DataArgumentationLayer", "128,96,16,2,2,synthetic:2,detectnet",
                                                    num_classes=2))
    solver = tmp_path / "solver.prototxt"
    solver.write_text('net: "%s"\nbase_lr: 1e-4\nweight_decay: 1e-6\ndisplay: 1\nmax_iter: %d\nsnapshot: %d\nsnapshot_prefix: "%s"\n%s'
                      % (net, max_iter, snapshot, tmp_path / "snap", extra))
    return str(solver)


def _solver(tmp_path, extra, **kw):
    if PYDIR not in sys.path:
        sys.path.insert(0, PYDIR)
    from fcn_object_detector_amd.solver import Solver
    return Solver(write_job(tmp_path, extra, **kw), device=0, log=None, autotune=False)


def _reseed(s, seed):
    random.seed(seed)
    s.py_layers[0][1]._color_rng = np.random.default_rng(seed)


@pytest.mark.parametrize("extra", ['type: "AdaDelta"\nmomentum: 0.95\ndelta: 1e-6\nlr_policy: "fixed"\n',
                                   'type: "Nesterov"\nmomentum: 0.9\nlr_policy: "multistep"\nstepvalue: 1\nstepvalue: 3\ngamma: 0.5\n'
                                   'clip_gradients: 10\niter_size: 2\n'], ids=["AdaDelta", "Nesterov-clip-iter_size"])
def test_snapshot_restore_step_equals_step_step(gpu, tmp_path, extra):
    a = _solver(tmp_path, extra, max_iter=100, snapshot=0)
    _reseed(a, 7)
    a.step(2)
    a.snapshot()
    b = _solver(tmp_path, extra, max_iter=100, snapshot=0)
    b.restore(str(tmp_path / "snap_iter_2.solverstate"))
    assert b.iter == 2
    ha, hb = a.engine.download_history(), b.engine.download_history()
    n = sum(len(v) for v in a.engine.download_params().values())
    assert len(ha) == len(hb) == (2 if "AdaDelta" in extra else 1) * n and all(np.array_equal(x, y) for x, y in zip(ha, hb))
    out = []
    for s in (a, b):
        _reseed(s, 99)
        out.append(s.step(1)["loss"])
    assert out[0] == out[1]
    pa, pb = a.engine.download_params(), b.engine.download_params()
    assert all(np.array_equal(x, y) for k in pa for x, y in zip(pa[k], pb[k]))
    # a state with the wrong number of history blobs is refused, not half loaded
    c = _solver(tmp_path, 'type: "Adam"\nmomentum: 0.9\n' if "AdaDelta" not in extra else 'type: "RMSProp"\n', max_iter=100, snapshot=0)
    with pytest.raises(ValueError, match="history"):
        c.restore(str(tmp_path / "snap_iter_2.solverstate"))
    for s in (a, b, c):
        s.close()


def test_two_identical_runs_give_identical_bits(gpu, tmp_path):
    extra = 'type: "Nesterov"\nmomentum: 0.9\nlr_policy: "poly"\npower: 1\nclip_gradients: 1\niter_size: 2\nregularization_type: "L1"\n'
    runs = []
    for _ in range(2):
        s = _solver(tmp_path, extra, max_iter=100, snapshot=0)
        _reseed(s, 21)
        losses = [s.step(1)["loss"] for _ in range(3)]
        runs.append((losses, s.engine.download_params(), s.engine.read_clip()))
        s.close()
    assert runs[0][0] == runs[1][0] and runs[0][2] == runs[1][2] and 0 < runs[0][2][0] <= 1.0
    assert all(np.array_equal(x, y) for k in runs[0][1] for x, y in zip(runs[0][1][k], runs[1][1][k]))


def test_caffe_train_with_an_edited_solver_file(gpu, tmp_path):
    """Nesterov, multistep with two stepvalues, clip_gradients and iter_size 2 through the `caffe train` tool: trains, snapshots, resumes."""
    solver = write_job(tmp_path, 'type: "Nesterov"\nmomentum: 0.9\nlr_policy: "multistep"\nstepvalue: 2\nstepvalue: 3\ngamma: 0.5\n'
                                 'clip_gradients: 10\niter_size: 2\n')
    env = dict(os.environ, PYTHONPATH=PYDIR + os.pathsep + os.environ.get("PYTHONPATH", ""), FCN_DATA_SEED="1")
    r = subprocess.run([sys.executable, CAFFE, "train", "--solver=%s" % solver, "--gpu=0"], capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    log = r.stderr
    assert 'type: "Nesterov"' in log and 'lr_policy: "multistep"' in log and "iter_size: 2" in log
    assert "Iteration 0, lr = 0.0001" in log and "Iteration 2, lr = 5e-05" in log and "Iteration 3, lr = 2.5e-05" in log
    assert log.count(", loss = ") == 4 and "Optimization Done." in log
    for it in (2, 4):
        for ext in (".caffemodel", ".solverstate"):
            assert os.path.getsize(str(tmp_path / ("snap_iter_%d%s" % (it, ext)))) > 1000
    os.remove(str(tmp_path / "snap_iter_4.caffemodel"))
    r2 = subprocess.run([sys.executable, CAFFE, "train", "-solver", solver, "-snapshot", str(tmp_path / "snap_iter_2.solverstate")],
                        capture_output=True, text=True, timeout=900, env=env)
    assert r2.returncode == 0, r2.stderr[-3000:]
    assert "Restoring previous solver status" in r2.stderr and "Iteration 2, loss = " in r2.stderr and "Iteration 1, loss = " not in r2.stderr
    assert os.path.isfile(str(tmp_path / "snap_iter_4.caffemodel"))
