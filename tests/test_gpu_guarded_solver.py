"""Guard-banded, poisoned-buffer parity of the solver entry points against the float64 restatement (tests/ref_solver64.py), -m gpu.

As in tests/test_gpu_guarded.py every buffer is a guarded allocation with 256 KiB red zones; the flat parameter, gradient and history
buffers are cut into segments with poisoned words between them (and behind the last one), which must be bit-identical afterwards and
must not reach a result.  fcn_solver_update_f32 runs several steps in a row on the device's own state, each step held to the
reference applied to the state the device had before it; fcn_grad_clip_f32 must give the same bits twice and float64's sum to 1e-6;
fcn_grad_accumulate_f32 is exact."""
import numpy as np
import pytest

import ref_solver64 as S
from fcn_object_detector_amd import lib as L
from gpu_util import Guards, poisoned

pytestmark = pytest.mark.gpu

U32 = 2.0 ** -24
KIND_NAMES = ("SGD", "NESTEROV", "ADAGRAD", "RMSPROP", "ADADELTA", "ADAM")


@pytest.fixture
def g(gpu):
    with Guards() as guards:
        yield guards


def worst(y, y64, allow):
    y = np.asarray(y, np.float64)
    r = np.where(np.isfinite(y), np.abs(y - y64) / allow, np.inf)
    i = int(np.argmax(r))
    return float(r[i]), i


def within(y, y64, allow, what):
    ratio, at = worst(y, y64, allow)
    print("BOUND %s %.3g" % (what, ratio))
    assert ratio <= 1.0, "%s: element %d is off by %.3g of its allowance" % (what, at, ratio)


def layout(counts, lr_mults, decay_mults, gaps=2, first=0):
    """Segments `gaps` poisoned words apart, the first at word `first`; the buffer is padded with poison to whole 16 bytes."""
    n = len(counts)
    segs = (L.SolverSeg * n)()
    off = first
    for i, cnt in enumerate(counts):
        segs[i].offset, segs[i].count, segs[i].lr_mult, segs[i].decay_mult = off, cnt, lr_mults[i], decay_mults[i]
        off += cnt + gaps
    total = (off - gaps + 3) // 4 * 4
    live = np.zeros(total, bool)
    for s in segs:
        live[s.offset:s.offset + s.count] = True
    return segs, live, total


def per_element(segs, total, field):
    out = np.zeros(total)
    for s in segs:
        out[s.offset:s.offset + s.count] = getattr(s, field)
    return out


def flat(rng, live, scale=1.0, positive=False):
    a = poisoned(live.size)
    v = rng.standard_normal(int(live.sum())) * scale
    a[live] = np.abs(v) if positive else v
    return a


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def solver_case(rng):
    segs, live, total = layout([5, 1003, 4, 37], (1.0, 0.0, 2.0, 0.5), (1.0, 1.0, 0.0, 2.0))
    assert total % 4 == 0 and not live[5:7].any() and not live[-1]
    return segs, live, total


HYPER = dict(rate=0.01, momentum=0.9, momentum2=0.999, rms_decay=0.97, delta=1e-6, weight_decay=5e-3)


def call_update(kind, wd, gd, h1d, h2d, sd, nseg, t, reg, grad_scale, clip_ptr, momentum):
    L.call("fcn_solver_update_f32", S.KINDS[kind], wd.ptr, gd.ptr, h1d.ptr, h2d.ptr if h2d is not None else None, sd.ptr, nseg, HYPER["rate"],
           momentum, HYPER["momentum2"], HYPER["rms_decay"], HYPER["delta"], HYPER["weight_decay"], L.REG_L1 if reg == "L1" else L.REG_L2, t,
           grad_scale, clip_ptr, None)


@pytest.mark.parametrize("clip", [None, 0.37])
@pytest.mark.parametrize("reg", ["L2", "L1"])
@pytest.mark.parametrize("kind", KIND_NAMES)
def test_solver_update_three_steps(g, kind, reg, clip):
    rng = np.random.default_rng(100 + 7 * S.KINDS[kind] + (reg == "L1") + 2 * (clip is not None))
    segs, live, total = solver_case(rng)
    two = kind in ("ADADELTA", "ADAM")
    momentum = 0.0 if kind in ("ADAGRAD", "RMSPROP") else HYPER["momentum"]
    grad_scale = 0.5
    w = flat(rng, live)
    h1 = flat(rng, live, 0.1, positive=kind not in ("SGD", "NESTEROV", "ADAM"))
    h2 = flat(rng, live, 0.01, positive=True) if two else None
    frozen = slice(segs[1].offset, segs[1].offset + segs[1].count)
    wd, h1d = g.put(w, at_end=True, name="w"), g.put(h1, at_end=True, name="h1")
    h2d = g.put(h2, at_end=True, name="h2") if two else None
    sd = g.put(np.frombuffer(bytes(segs), np.uint8), name="segments")
    cd = g.put(np.array([clip], np.float32), name="clip word") if clip is not None else None
    lr_mult, decay_mult = per_element(segs, total, "lr_mult"), per_element(segs, total, "decay_mult")
    moves = live.copy()
    moves[frozen] = False
    f = S.f32
    hyp = dict(rate=f(HYPER["rate"]), lr_mult=lr_mult, momentum=f(momentum), momentum2=f(HYPER["momentum2"]), rms_decay=f(HYPER["rms_decay"]),
               delta=f(HYPER["delta"]))
    cf = f(clip) if clip is not None else 1.0
    z = lambda a: np.where(live, a, 0).astype(np.float64)
    for step in range(3):
        t = step + 1
        gr = flat(rng, live, 2.0)
        gd = g.put(gr, at_end=True, name="g step %d" % step)
        call_update(kind, wd, gd, h1d, h2d, sd, len(segs), t, reg, grad_scale, cd.ptr if cd is not None else None, momentum)
        w_new, h1_new = wd.read((total,)), h1d.read((total,))
        h2_new = h2d.read((total,)) if two else None
        # outside the segments, in the lr_mult = 0 segment and in the gradient: bit-identical
        for new, old in ((w_new, w), (h1_new, h1)) + (((h2_new, h2),) if two else ()):
            assert np.array_equal(bits(new)[~moves], bits(old)[~moves])
        assert np.array_equal(bits(gd.read((total,))), bits(gr))
        # the reference on the state the device had before this step; the allowance = what the rounding of g' (2 u of its two
        # terms) does to each output, by evaluating the rule at g' +- that, plus a few ulps of the output's own operands
        r = z(w) if reg == "L2" else np.sign(z(w))
        term_g, term_r = z(gr) * grad_scale * cf, f(HYPER["weight_decay"]) * decay_mult * r
        gg = term_g + term_r
        eg = 2 * U32 * (np.abs(term_g) + np.abs(term_r))
        assert np.allclose(gg, S.effective_gradient(z(w), z(gr), f(HYPER["weight_decay"]), decay_mult, grad_scale, cf, reg), rtol=1e-15, atol=0)
        h2_in = z(h2) if two else None
        ref = S.update_from_gradient(kind, z(w), gg, z(h1), h2_in, t=t, **hyp)
        lo = S.update_from_gradient(kind, z(w), gg - eg, z(h1), h2_in, t=t, **hyp)
        hi = S.update_from_gradient(kind, z(w), gg + eg, z(h1), h2_in, t=t, **hyp)
        prop = [np.maximum(np.abs(a - c), np.abs(b - c)) if c is not None else None for a, b, c in zip(lo, hi, ref)]
        mag_w = np.abs(z(w)) + np.abs(ref[0] - z(w)) + (2 * np.abs(ref[1]) + np.abs(z(h1)) if kind == "NESTEROV" else 0)
        within(w_new[moves], ref[0][moves], (prop[0] + 4 * U32 * mag_w)[moves] + 1e-37, "%s %s w step %d" % (kind, reg, step))
        within(h1_new[moves], ref[1][moves], (prop[1] + 4 * U32 * (np.abs(ref[1]) + np.abs(z(h1))))[moves] + 1e-37, "%s %s h1 step %d" % (kind, reg, step))
        if two:
            within(h2_new[moves], ref[2][moves], (prop[2] + 8 * U32 * (np.abs(ref[2]) + np.abs(z(h2))))[moves] + 1e-37,
                   "%s %s h2 step %d" % (kind, reg, step))
        assert np.abs(w_new[moves] - w[moves]).max() > 1e-5      # (the step moved the weights: the bounds above compare something)
        w, h1, h2 = w_new, h1_new, h2_new


@pytest.mark.parametrize("kind", ["SGD", "ADAM"])
def test_sgd_and_adam_through_the_new_entry_are_bit_identical(g, kind):
    rng = np.random.default_rng(7)
    segs, live, total = solver_case(rng)
    state = [flat(rng, live), flat(rng, live, 0.1), flat(rng, live, 0.01, positive=True)]
    old = [g.put(a, at_end=True) for a in state]
    new = [g.put(a, at_end=True) for a in state]
    sd = g.put(np.frombuffer(bytes(segs), np.uint8), name="segments")
    for step in range(3):
        gr = flat(rng, live, 2.0)
        gd = g.put(gr, at_end=True, name="g")
        if kind == "SGD":
            L.call("fcn_sgd_update_f32", old[0].ptr, gd.ptr, old[1].ptr, sd.ptr, len(segs), 0.01, 0.9, 5e-3, 0.25, None)
        else:
            L.call("fcn_adam_update_f32", old[0].ptr, gd.ptr, old[1].ptr, old[2].ptr, sd.ptr, len(segs), 0.01, 0.9, 0.999, 1e-6, 5e-3, step + 1, 0.25, None)
        L.call("fcn_solver_update_f32", S.KINDS[kind], new[0].ptr, gd.ptr, new[1].ptr, new[2].ptr if kind == "ADAM" else None, sd.ptr, len(segs),
               0.01, 0.9, 0.999, 0.99, 1e-6, 5e-3, L.REG_L2, step + 1, 0.25, None, None)
        for a, b in zip(old, new):
            assert np.array_equal(bits(a.read((total,))), bits(b.read((total,)))), step
    assert not np.array_equal(bits(new[0].read((total,))), bits(state[0]))


def test_a_clip_word_of_one_changes_nothing(g):
    rng = np.random.default_rng(8)
    segs, live, total = solver_case(rng)
    w, h, gr = flat(rng, live), flat(rng, live, 0.1), flat(rng, live, 2.0)
    sd = g.put(np.frombuffer(bytes(segs), np.uint8), name="segments")
    gd, one = g.put(gr, at_end=True), g.put(np.array([1.0], np.float32))
    out = []
    for clip in (None, one.ptr):
        wd, hd = g.put(w, at_end=True), g.put(h, at_end=True)
        L.call("fcn_solver_update_f32", S.KINDS["NESTEROV"], wd.ptr, gd.ptr, hd.ptr, None, sd.ptr, len(segs), 0.01, 0.9, 0.999, 0.99, 1e-8, 5e-3,
               L.REG_L2, 1, 0.5, clip, None)
        out.append((wd.read((total,)), hd.read((total,))))
    assert np.array_equal(bits(out[0][0]), bits(out[1][0])) and np.array_equal(bits(out[0][1]), bits(out[1][1]))


# ---- clip factor ----------------------------------------------------------------------------------------------------------------
def clip_layout(n):
    """n elements in up to three segments that start at words 3, then wherever a 1- / 2-word gap leaves them (unaligned heads and tails)."""
    if n == 1:
        return layout([1], (1.0,), (1.0,), first=3)
    a = max(1, n // 7)
    b = max(1, (n - a) // 3)
    return layout([a, b, n - a - b], (1.0, 0.0, 2.0), (1.0, 1.0, 1.0), gaps=1, first=3)


@pytest.mark.parametrize("n", [1, 1000, 2 ** 20 + 3, 15_000_000])
def test_grad_clip_sum_of_squares(g, n):
    rng = np.random.default_rng(n % 1000)
    segs, live, total = clip_layout(n)
    assert int(live.sum()) == n
    gr = poisoned(total)
    gr[live] = (rng.standard_normal(n) * 0.01).astype(np.float32)
    want = float(np.sum(gr[live].astype(np.float64) ** 2))
    norm = np.sqrt(want)
    gd = g.put(gr, at_end=True, name="g")
    sd = g.put(np.frombuffer(bytes(segs), np.uint8), name="segments")
    nws = int(L.load().fcn_grad_clip_workspace_bytes())
    runs = []
    for rep in range(2):
        ws, out = g.put(nws, name="workspace"), g.put(np.zeros(2, np.float32), at_end=True, name="clip, sumsq")
        L.call("fcn_grad_clip_f32", gd.ptr, sd.ptr, len(segs), float(0.5 * norm), 1.0, out.ptr, out.ptr + 4, ws.ptr, None)
        runs.append(out.read((2,)))
    assert np.array_equal(bits(runs[0]), bits(runs[1])), "two runs differ"
    clip, sumsq = float(runs[0][0]), float(runs[0][1])
    assert abs(sumsq - want) <= 1e-6 * want, (sumsq, want)
    ref = S.clip_factor(want, S.f32(0.5 * norm))
    assert abs(clip - ref) <= 4 * U32 * ref and 0.49 < clip < 0.51
    assert np.array_equal(bits(gd.read((total,))), bits(gr))
    # below the threshold (and exactly at it, as far as float32 can say): the word is exactly 1.0; norm_scale scales the norm
    out = g.put(np.zeros(1, np.float32), name="clip")
    ws = g.put(nws, name="workspace")
    for thresh, ns, expect in ((2.0 * norm, 1.0, 1.0), (0.6 * norm, 0.5, 1.0), (0.25 * norm, 0.5, None)):
        L.call("fcn_grad_clip_f32", gd.ptr, sd.ptr, len(segs), float(thresh), ns, out.ptr, None, ws.ptr, None)
        got = float(out.read((1,))[0])
        if expect is not None:
            assert got == 1.0, (thresh, ns, got)
        else:
            ref = S.clip_factor(want, S.f32(thresh), ns)
            assert abs(got - ref) <= 4 * U32 * ref and 0.49 < got < 0.51


def test_grad_clip_of_a_zero_gradient_is_one(g):
    segs, live, total = clip_layout(1000)
    gr = poisoned(total)
    gr[live] = 0
    gd, sd = g.put(gr, at_end=True), g.put(np.frombuffer(bytes(segs), np.uint8))
    ws, out = g.put(int(L.load().fcn_grad_clip_workspace_bytes())), g.put(np.full(2, 7.0, np.float32))
    L.call("fcn_grad_clip_f32", gd.ptr, sd.ptr, len(segs), 1e-3, 1.0, out.ptr, out.ptr + 4, ws.ptr, None)
    assert out.read((2,)).tolist() == [1.0, 0.0]


def test_clip_word_feeds_the_update(g):
    """The two calls a clipped step makes: the factor stays on the device, and the update equals the reference with that factor."""
    rng = np.random.default_rng(9)
    segs, live, total = solver_case(rng)
    w, h, gr = flat(rng, live), flat(rng, live, 0.1), flat(rng, live, 2.0)
    wd, hd, gd = g.put(w, at_end=True), g.put(h, at_end=True), g.put(gr, at_end=True)
    sd = g.put(np.frombuffer(bytes(segs), np.uint8), name="segments")
    ws, out = g.put(int(L.load().fcn_grad_clip_workspace_bytes())), g.put(np.zeros(2, np.float32))
    L.call("fcn_grad_clip_f32", gd.ptr, sd.ptr, len(segs), 3.0, 0.5, out.ptr, out.ptr + 4, ws.ptr, None)
    L.call("fcn_solver_update_f32", S.KINDS["SGD"], wd.ptr, gd.ptr, hd.ptr, None, sd.ptr, len(segs), 0.01, 0.9, 0.999, 0.99, 1e-8, 0.0, L.REG_L2, 1,
           0.5, out.ptr, None)
    z = lambda a: np.where(live, a, 0).astype(np.float64)
    cf = S.clip_factor(float(np.sum(z(gr) ** 2)), 3.0, 0.5)
    assert cf < 0.2 and abs(float(out.read((2,))[0]) - cf) <= 4 * U32 * cf
    lr_mult = per_element(segs, total, "lr_mult")
    w64, h64, _ = S.update("SGD", z(w), z(gr), z(h), None, S.f32(0.01), lr_mult, 0.0, momentum=S.f32(0.9), grad_scale=0.5, clip=cf)
    moves = live & (lr_mult != 0)
    within(hd.read((total,))[moves], h64[moves], 16 * U32 * (np.abs(h64) + np.abs(z(h)))[moves] + 1e-37, "clipped sgd history")
    within(wd.read((total,))[moves], w64[moves], 16 * U32 * (np.abs(w64) + np.abs(h64))[moves] + 1e-37, "clipped sgd weights")


# ---- accumulation ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count,at_end", [(4096, True), (1003, False), (3, False), (2 ** 20 + 5, False)])
def test_grad_accumulate_three_buffers(g, count, at_end):
    rng = np.random.default_rng(count)
    gs = [rng.standard_normal(count).astype(np.float32) for _ in range(3)]
    acc = g.put(4 * count, at_end=at_end, name="acc")      # starts as poison: `first` must overwrite, not add
    for i, a in enumerate(gs):
        gd = g.put(a, at_end=at_end, name="g%d" % i)
        L.call("fcn_grad_accumulate_f32", acc.ptr, gd.ptr, count, int(i == 0), None)
        assert np.array_equal(bits(gd.read((count,))), bits(a))
    want = (gs[0] + gs[1]) + gs[2]
    assert np.array_equal(bits(acc.read((count,))), bits(want))
