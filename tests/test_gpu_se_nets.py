"""SE-ResNet-50 (models.se_resnet, both forms) through the public surface, -m gpu, against torch in float64 on the CPU
(tests/torch_se_ref.py), in the style of tests/test_gpu_resnet.py.

The net: se_resnet(depth=50, width_div=8, size=64, batch=2, num_classes=10, reduction=4) - block widths 32 .. 256 and squeeze widths
8 .. 64, whole 16-byte groups of floats and of halves - from a prototxt and a caffemodel through caffe.Net.  The biases of the excite
layers are seeded so that the gates spread over (0.1, 0.9), and the second image is three times the contrast of the first so that
the gates differ between the two images; that is asserted on the reference first
(a gate of 0.5 everywhere, or the same for both images, would hide a kernel that takes the wrong row of the gate).
float32: every block's gate, scaled branch (the top of the gated Scale, which the fused launch never writes: net.blobs fills it on
demand) and output, and prob, at the project's rel_err < 1e-4; form "axpy" on the same weights gives what form "scale" gives.
One SGD step in TRAIN through caffe.SGDSolver: the loss within 1e-4 relative and every blob after the update at rel_err < 1e-4 against
w - lr * lr_mult * dw from autograd in float64 (the BatchNorm blobs against Caffe's moving-average step), the device's ReLU masks
adopted in the reference's backward pass as tests/test_gpu_resnet.py does; the gradients of the squeeze and excite layers - what the
gate's two gradient launches feed - are held, in addition, to that file's rule max(5e-4, 4 x torch float32's own error).
Halves: against float64 rounded where the engine rounds (torch_se_ref.half_reference).  Threshold, measured and not chosen, by the rule
of tests/test_gpu_tconv_f16_nets.py: the float32 run of the reference with the same rounding against the float64 one, both forms, three
seeds - worst rel_err 1.62e-3 (a rounding that falls the other way in float32 travels through 16 blocks), measured again for this
file's seed without a GPU by tests/test_se_nets_ref.py.  4 x that is 6.5e-3, above the project's bound for half-float nets, so that bound
holds: TOL_F16 = 5e-3 (the constants live in tests/torch_se_ref.py, which the part without a GPU shares)."""
import sys

import numpy as np
import pytest
import torch

from conftest import PYCAFFE, rel_err
from fcn_object_detector_amd import proto
from torch_se_ref import BLOCKS, TOL, TOL_F16, as_form, as_torch, gates_spread, half_reference, se_case, torch_se_net

pytestmark = pytest.mark.gpu
F32 = np.float32
NAMES = [b + s for b in BLOCKS for s in ("_prob", "/scale", "")] + ["prob"]


def _caffe():
    if PYCAFFE not in sys.path:
        sys.path.insert(0, PYCAFFE)
    import caffe
    return caffe


def load(tmp_path, txt, spec, params, tag, **kw):
    caffe = _caffe()
    path, weights = str(tmp_path / (tag + ".prototxt")), str(tmp_path / (tag + ".caffemodel"))
    open(path, "w").write(txt)
    proto.write_caffemodel(weights, [(l.name, l.type, params[l.name]) for l in spec.param_layers()])
    caffe.set_device(0)
    caffe.set_mode_gpu()
    return caffe.Net(path, weights, caffe.TEST, **kw)


@pytest.fixture(scope="module")
def case():
    """The float64 reference of the DEPLOY net, computed once and shared."""
    txt, spec, params, x = se_case("DEPLOY", "scale")
    with torch.no_grad():
        ref = torch_se_net(spec, as_torch(params), x)
    gates_spread(ref)
    return txt, spec, params, x, ref


def test_float32_forward_of_both_forms(gpu, tmp_path, monkeypatch, case):
    monkeypatch.setenv("FCN_AUTOTUNE", "0")
    txt, spec, params, x, ref = case
    got = {}
    for form in ("scale", "axpy"):
        ftxt, fspec, _p, _x = se_case("DEPLOY", form)
        assert ("Axpy" in ftxt) == (form == "axpy")
        net = load(tmp_path, ftxt, fspec, as_form(params, fspec), form)
        eng = net._engine
        gate_ops = [op for op in eng.ops if op.kind == "scale_gate"]
        assert len(gate_ops) == 16 and all(op.name == "%s/scale+%s+%s/relu" % (b, b, b) for op, b in zip(gate_ops, BLOCKS))
        assert sorted(eng._lazy_blob_ops) == sorted(b + "/scale" for b in BLOCKS)
        net.blobs["data"].data[...] = x["data"]
        out = net.forward()
        got[form] = {n: np.array(net.blobs[n].data).reshape(ref[n].shape) for n in NAMES}
        for n in NAMES:
            err = rel_err(got[form][n], ref[n].numpy())
            print("SE %s %s %.3g" % (form, n, err))
            assert err < TOL, (form, n, err)
        assert rel_err(out["prob"], ref["prob"].numpy()) < TOL
        # graph replay and a forward without a graph: the same bytes
        a = {n: eng.read_blob(n).copy() for n in BLOCKS + ["prob"]}
        eng.forward(use_graph=True)
        b = {n: eng.read_blob(n).copy() for n in BLOCKS + ["prob"]}
        eng.forward(use_graph=False)
        c = {n: eng.read_blob(n).copy() for n in BLOCKS + ["prob"]}
        assert all(a[n].tobytes() == b[n].tobytes() == c[n].tobytes() for n in a), form
    for n in NAMES:
        assert rel_err(got["axpy"][n], got["scale"][n]) < TOL, n


def test_replay_and_eager_give_the_same_bytes(gpu, tmp_path, monkeypatch, case):
    """Two forwards through the captured graph and two with FCN_NO_GRAPH=1 (plain launches) on one net - one plan, as tests/test_gpu_ssd_nets.py
    compares them: two nets may be tuned to different tiles, whose sums round differently."""
    txt, spec, params, x, ref = case
    net = load(tmp_path, txt, spec, params, "replay")
    outs = []
    for no_graph in ("0", "1"):
        monkeypatch.setenv("FCN_NO_GRAPH", no_graph)
        for _ in range(2):
            net.blobs["data"].data[...] = x["data"]
            net.forward()
            outs.append({n: np.array(net.blobs[n].data).copy() for n in BLOCKS + ["prob"]})
    assert net._engine.graph_io is not None
    for o in outs[1:]:
        assert [n for n in o if o[n].tobytes() != outs[0][n].tobytes()] == []


@pytest.mark.parametrize("form", ["scale", "axpy"])
def test_half_float_forward(gpu, tmp_path, monkeypatch, form):
    monkeypatch.setenv("FCN_AUTOTUNE", "0")
    txt, spec, params, x = se_case("DEPLOY", form)
    ref, half = half_reference(spec, params, x)
    net = load(tmp_path, txt, spec, params, "h" + form, dtype="f16")
    eng = net._engine
    assert eng.f16 and {n for n, b in eng.blobs.items() if b.esize == 2} == half
    assert all(eng.blobs[b + "_prob"].esize == 4 and eng.blobs[b].esize == 2 and eng.blobs[b + "/scale"].esize == 2 for b in BLOCKS)
    assert len([op for op in eng.ops if op.kind == "scale_gate"]) == 16
    net.blobs["data"].data[...] = x["data"]
    out = net.forward()
    for n in [b + s for b in BLOCKS for s in ("_prob", "")] + ["prob"]:
        err = rel_err(eng.read_blob(n).reshape(ref[n].shape), ref[n].numpy())
        print("SE16 %s %s %.3g" % (form, n, err))
        assert err < TOL_F16, (n, err)
    assert out["prob"].dtype == F32 and abs(float(out["prob"].sum()) - 2.0) < 1e-3
    a = eng.read_blob("prob").copy()
    eng.forward(use_graph=False)
    assert a.tobytes() == eng.read_blob("prob").tobytes()


@pytest.mark.parametrize("form", ["scale", "axpy"])
def test_one_solver_step(gpu, tmp_path, monkeypatch, form):
    monkeypatch.setenv("FCN_AUTOTUNE", "0")
    caffe = _caffe()
    txt, spec, params, x = se_case("TRAIN", form)
    lr = 0.01
    train, job = tmp_path / "train.prototxt", tmp_path / "solver.prototxt"
    train.write_text(txt)
    job.write_text('train_net: "%s"\nbase_lr: %g\nmomentum: 0\nweight_decay: 0\nlr_policy: "fixed"\nmax_iter: 10\nsnapshot_prefix: "%s"\n'
                   % (train, lr, tmp_path / "snap"))
    s = caffe.SGDSolver(str(job), log=None, autotune=False)
    eng = s.engine
    assert eng.spec.scale_gate and [op.kind for op in eng.ops].count("scale_gate") == 16
    bk = [op.kind for op in eng.bwd_ops]
    assert bk.count("scale_gate_bwd") == 32
    for l in spec.param_layers():
        eng.set_params(l.name, params[l.name])
    for k, v in x.items():
        eng.host_array(k)[...] = v
    out = s.step(1)
    updates = {}
    with torch.no_grad():
        fwd = torch_se_net(spec, as_torch(params), x, updates=updates)
    want = float(fwd["total_loss"])
    print("SESTEP %s loss %.6g want %.6g" % (form, out["loss"], want))
    assert abs(out["loss"] - want) < 1e-4 * abs(want)
    masks = {l.name: eng.read_blob(l.tops[0]) > 0 for l in spec.layers if l.type == "ReLU"}
    P = as_torch(params, grad=True)
    torch_se_net(spec, P, x, relu_masks=masks)["total_loss"].backward()
    P32 = as_torch(params, grad=True, dtype=torch.float32)
    torch_se_net(spec, P32, x, relu_masks=masks, dtype=torch.float32)["total_loss"].backward()
    now, grads = eng.download_params(), eng.download_grads()
    worst = (0.0, None)
    for l in spec.param_layers():
        for i, w0 in enumerate(params[l.name]):
            if l.type == "BatchNorm":
                expect = updates[l.name][i]
            else:
                mult = l.lr_mult[i] if i < len(l.lr_mult) else 1.0
                expect = np.asarray(w0, np.float64) - lr * mult * P[l.name][i].grad.numpy()
            err = rel_err(now[l.name][i], expect)
            worst = max(worst, (err, "%s[%d]" % (l.name, i)))
            assert err < TOL, "blob %d of %s after the step: %.3g" % (i, l.name, err)
            if l.name.endswith(("_1x1_down", "_1x1_up")):
                own = rel_err(P32[l.name][i].grad.numpy(), P[l.name][i].grad.numpy())
                gerr = rel_err(grads[l.name][i], P[l.name][i].grad.numpy())
                print("SEGRAD %s %s[%d] %.3g (torch float32: %.3g)" % (form, l.name, i, gerr, own))
                assert gerr < max(5e-4, 4 * own), "gradient %d of %s: %.3g (torch float32: %.3g)" % (i, l.name, gerr, own)
    print("SESTEP %s worst updated blob %.3g at %s" % (form, worst[0], worst[1]))
    s.close()
