"""Solver settings without a GPU: SolverParams parses every solver type (both spellings), every lr_policy gives Caffe's rate,
Caffe's constraints are ValueErrors naming the field, a .solverstate carries N or 2N histories, and the new solver entry points
refuse bad arguments before any HIP call (fake non-null 16-byte-aligned addresses are enough: nothing is launched here)."""
import math

import numpy as np
import pytest

import ref_solver64 as S
from fcn_object_detector_amd import lib as L
from fcn_object_detector_amd import proto
from fcn_object_detector_amd.train import SolverParams

E_ARG, E_ALIGN = 1, 2
W, G, H1, H2, SEG, WS, CLIP = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 0x60000, 0x70000      # never dereferenced

TYPES = [("SGD", "SGD", 1), ("Nesterov", "NESTEROV", 1), ("AdaGrad", "ADAGRAD", 1), ("RMSProp", "RMSPROP", 1), ("AdaDelta", "ADADELTA", 2),
         ("Adam", "ADAM", 2)]


def params(text):
    return SolverParams(proto.parse_text(text))


# ---- types ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,kind,hist", TYPES)
def test_both_spellings_of_every_type(name, kind, hist):
    for text in ('type: "%s"' % name, 'type: "%s"' % name.lower(), 'type: "%s"' % name.upper(), "solver_type: %s" % kind):
        p = params('net: "n.prototxt"\n%s\nbase_lr: 0.01\n' % text)
        assert p.kind == kind and p.histories == hist, text
    assert SolverParams(solver_type=kind).kind == kind and SolverParams(type=name).kind == kind
    assert L.SOLVER_KINDS[kind] == S.KINDS[kind]


def test_defaults_are_caffes():
    p = SolverParams()
    assert (p.kind, p.lr_policy, p.regularization_type) == ("SGD", "fixed", "L2")
    assert (p.momentum, p.delta, p.rms_decay, p.clip_gradients, p.iter_size, p.power, p.stepvalue) == (0.0, 1e-8, 0.99, -1.0, 1, 0.0, [])


def test_new_fields_are_read_from_the_file():
    p = params('type: "AdaDelta"\ndelta: 1e-6\nmomentum: 0.95\nclip_gradients: 10\nregularization_type: "L1"\niter_size: 4\n'
               'lr_policy: "multistep"\nstepvalue: 30\nstepvalue: 10\ngamma: 0.5\npower: 0.75\nrms_decay: 0.9\n')
    assert (p.kind, p.delta, p.momentum, p.clip_gradients, p.regularization_type, p.iter_size) == ("ADADELTA", 1e-6, 0.95, 10.0, "L1", 4)
    assert p.stepvalue == [10, 30] and p.power == 0.75 and p.rms_decay == 0.9


@pytest.mark.parametrize("text,field", [
    ('type: "AdaGrad"\nmomentum: 0.9\n', "momentum"),
    ('type: "RMSProp"\nmomentum: 0.5\n', "momentum"),
    ("solver_type: RMSPROP\nrms_decay: 1.0\n", "rms_decay"),
    ("momentum: 1.5\n", "momentum"),
    ('lr_policy: "multistep"\n', "stepvalue"),
    ('lr_policy: "poly"\npower: 1\nmax_iter: 0\n', "max_iter"),
    ('lr_policy: "step"\nstepsize: 0\n', "stepsize"),
    ('lr_policy: "cosine"\n', "lr_policy"),
    ('type: "LBFGS"\n', "type"),
    ('regularization_type: "L3"\n', "regularization_type"),
    ("iter_size: 0\n", "iter_size"),
])
def test_caffes_constraints_are_value_errors_naming_the_field(text, field):
    with pytest.raises(ValueError, match=field):
        params(text)


# ---- learning-rate policies -----------------------------------------------------------------------------------------------------
def test_fixed_and_step_are_unchanged():
    assert [SolverParams(base_lr=0.5).rate(i) for i in (0, 7)] == [0.5, 0.5]
    p = SolverParams(base_lr=1e-4, lr_policy="step", gamma=0.5, stepsize=4)
    assert [p.rate(i) for i in (0, 3, 4, 8)] == [1e-4, 1e-4, 5e-5, 2.5e-5]


def test_multistep_counts_the_stepvalues_passed():
    p = params('base_lr: 1.0\nlr_policy: "multistep"\ngamma: 0.1\nstepvalue: 3\nstepvalue: 5\n')
    got = [p.rate(i) for i in range(7)]
    assert got == pytest.approx([1, 1, 1, 0.1, 0.1, 0.01, 0.01], rel=1e-15)
    assert p.rate(1000) == pytest.approx(0.01)      # stateless: a run resumed past both values gets the same rate


def test_poly_reaches_zero_at_max_iter():
    p = SolverParams(base_lr=0.02, lr_policy="poly", power=2.0, max_iter=10)
    assert p.rate(0) == 0.02 and p.rate(5) == pytest.approx(0.02 * 0.25) and p.rate(10) == 0.0
    assert SolverParams(base_lr=0.02, lr_policy="poly", power=0.5, max_iter=4).rate(3) == pytest.approx(0.01)


def test_exp_inv_sigmoid_by_hand():
    assert SolverParams(base_lr=2.0, lr_policy="exp", gamma=0.5).rate(3) == pytest.approx(0.25)
    assert SolverParams(base_lr=1.0, lr_policy="inv", gamma=1.0, power=2.0).rate(1) == pytest.approx(0.25)
    assert SolverParams(base_lr=1.0, lr_policy="inv", gamma=1e-4, power=0.75).rate(10000) == pytest.approx(2.0 ** -0.75)
    p = SolverParams(base_lr=1.0, lr_policy="sigmoid", gamma=-0.5, stepsize=10)
    assert p.rate(10) == pytest.approx(0.5) and p.rate(12) == pytest.approx(1 / (1 + math.e)) and p.rate(0) > 0.99


@pytest.mark.parametrize("policy", SolverParams.POLICIES)
def test_every_policy_equals_the_float64_restatement(policy):
    kw = dict(base_lr=0.013, gamma=0.3 if policy != "sigmoid" else -0.2, power=1.5, stepsize=3, stepvalue=[2, 6, 7], max_iter=12)
    p = SolverParams(lr_policy=policy, **kw)
    for it in range(13):
        assert p.rate(it) == pytest.approx(S.rate(policy, it, **kw), rel=1e-14, abs=1e-300), it


# ---- the float64 restatement itself: known answers computed by hand -------------------------------------------------------------
def test_update_rules_known_answers():
    w, g, h = np.array([1.0]), np.array([0.5]), np.array([0.2])
    # g' = 0.5 * 2 * 0.5 + 0.1 * 1 = 0.6 (L2), 0.5 + 0.1 * sign(1) = 0.6 (L1): the same by construction; lr = 0.1 * 2
    common = dict(rate=0.1, lr_mult=2.0, weight_decay=0.1, grad_scale=2.0, clip=0.5)
    for reg in ("L2", "L1"):
        w2, h2, _ = S.update("SGD", w, g, h, None, momentum=0.5, reg=reg, **common)
        assert w2[0] == pytest.approx(1 - 0.22) and h2[0] == pytest.approx(0.22)                      # h = 0.5*0.2 + 0.2*0.6
    w2, h2, _ = S.update("NESTEROV", w, g, h, None, momentum=0.5, **common)
    assert h2[0] == pytest.approx(0.22) and w2[0] == pytest.approx(1 - (1.5 * 0.22 - 0.5 * 0.2))
    w2, h2, _ = S.update("ADAGRAD", w, g, np.array([0.64]), None, delta=0.0, **common)
    assert h2[0] == pytest.approx(1.0) and w2[0] == pytest.approx(1 - 0.2 * 0.6 / 1.0)
    w2, h2, _ = S.update("RMSPROP", w, g, np.array([1.0]), None, rms_decay=0.75, delta=0.0, **common)
    assert h2[0] == pytest.approx(0.75 + 0.25 * 0.36) and w2[0] == pytest.approx(1 - 0.2 * 0.6 / math.sqrt(0.84))
    w2, a2, b2 = S.update("ADADELTA", w, g, np.array([0.0]), np.array([0.09]), momentum=0.5, delta=0.0, **common)
    u = 0.6 * math.sqrt(0.09 / 0.18)                                                                  # h1 = 0.5 * 0.36
    assert a2[0] == pytest.approx(0.18) and b2[0] == pytest.approx(0.045 + 0.5 * u * u) and w2[0] == pytest.approx(1 - 0.2 * u)
    w2, m2, v2 = S.update("ADAM", w, g, np.array([0.0]), np.array([0.0]), momentum=0.9, momentum2=0.99, delta=0.0, t=1, **common)
    assert m2[0] == pytest.approx(0.06) and v2[0] == pytest.approx(0.0036) and w2[0] == pytest.approx(1 - 0.2)      # first Adam step: lr * sign
    assert S.effective_gradient([-2.0, 0.0], [0.0, 0.0], 0.1, 1.0, reg="L1").tolist() == [-0.1, 0.0]


def test_clip_factor_known_answers():
    assert S.clip_factor(25.0, 10.0) == 1.0 and S.clip_factor(100.0, 10.0) == 1.0 and S.clip_factor(400.0, 10.0) == 0.5
    assert S.clip_factor(400.0, 10.0, norm_scale=0.5) == 1.0 and S.clip_factor(1600.0, 10.0, norm_scale=0.5) == 0.5
    assert S.clip_factor(1e30, -1.0) == 1.0 and S.clip_factor(0.0, 1.0) == 1.0


# ---- .solverstate ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("copies", [1, 2])
def test_solverstate_round_trip_with_n_and_2n_histories(copies):
    rng = np.random.default_rng(3)
    shapes = [(4, 3, 3, 3), (4,), (2, 4, 1, 1), (2,)]
    hist = [rng.standard_normal(s).astype(np.float32) for _ in range(copies) for s in shapes]
    it, back, learned = proto.unpack_solverstate(proto.pack_solverstate(17, hist, learned_net="snap_iter_17.caffemodel"), with_learned_net=True)
    assert it == 17 and learned == "snap_iter_17.caffemodel" and len(back) == copies * len(shapes)
    for a, b in zip(hist, back):
        assert a.shape == tuple(b.shape) and np.array_equal(a, b)


# ---- argument checks of the new entry points ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    return L.load()


def err(lib):
    return lib.fcn_last_error_string().decode()


def update(lib, kind=1, w=W, g=G, h1=H1, h2=H2, segs=SEG, nseg=3, rate=0.01, momentum=0.9, momentum2=0.999, rms_decay=0.99, delta=1e-8,
           wd=5e-4, reg=0, t=1, grad_scale=1.0, clip=None):
    return lib.fcn_solver_update_f32(kind, w, g, h1, h2, segs, nseg, rate, momentum, momentum2, rms_decay, delta, wd, reg, t, grad_scale, clip, None)


def clip(lib, g=G, segs=SEG, nseg=3, c=10.0, ns=1.0, out=CLIP, sumsq=None, ws=WS):
    return lib.fcn_grad_clip_f32(g, segs, nseg, c, ns, out, sumsq, ws, None)


@pytest.mark.parametrize("kw", [dict(w=None), dict(g=None), dict(h1=None), dict(segs=None), dict(kind=4, h2=None), dict(kind=5, h2=None),
                                dict(nseg=0), dict(nseg=-3), dict(kind=6), dict(kind=-1), dict(momentum=1.0), dict(momentum=-0.1),
                                dict(momentum=float("nan")), dict(rms_decay=1.0), dict(rms_decay=-0.5), dict(reg=2),
                                dict(kind=5, momentum2=1.0), dict(kind=5, t=0)])
def test_solver_update_refuses_bad_arguments(lib, kw):
    assert update(lib, **kw) == E_ARG, kw
    assert err(lib).startswith("solver_update")


@pytest.mark.parametrize("kw", [dict(w=W + 4), dict(g=G + 8), dict(h1=H1 + 4), dict(kind=4, h2=H2 + 12), dict(segs=SEG + 8), dict(clip=CLIP + 2)])
def test_solver_update_refuses_misaligned_pointers(lib, kw):
    assert update(lib, **kw) == E_ALIGN, kw


@pytest.mark.parametrize("kw", [dict(g=None), dict(segs=None), dict(out=None), dict(ws=None), dict(nseg=0), dict(c=0.0), dict(c=-1.0), dict(ns=0.0)])
def test_grad_clip_refuses_bad_arguments(lib, kw):
    assert clip(lib, **kw) == E_ARG, kw


@pytest.mark.parametrize("kw", [dict(g=G + 4), dict(segs=SEG + 8), dict(ws=WS + 8), dict(out=CLIP + 1), dict(sumsq=CLIP + 6)])
def test_grad_clip_refuses_misaligned_pointers(lib, kw):
    assert clip(lib, **kw) == E_ALIGN, kw


def test_grad_clip_workspace_query(lib):
    n = int(lib.fcn_grad_clip_workspace_bytes())
    assert n > 0 and n % 16 == 0


def test_grad_accumulate_refuses_bad_arguments(lib):
    assert lib.fcn_grad_accumulate_f32(None, G, 16, 1, None) == E_ARG
    assert lib.fcn_grad_accumulate_f32(W, None, 16, 0, None) == E_ARG
    assert lib.fcn_grad_accumulate_f32(W, G, 0, 0, None) == E_ARG
    assert lib.fcn_grad_accumulate_f32(W + 4, G, 16, 0, None) == E_ALIGN
    assert lib.fcn_grad_accumulate_f32(W, G + 8, 16, 0, None) == E_ALIGN
