"""fcn_avepool_bwd_f32 without a GPU: the symbol and its prototype, every refusal of its contract (all of them precede the first HIP
call, so the pointers below are never dereferenced), and the float64 reference the guarded GPU test compares against, held to torch."""
import numpy as np
import pytest

import ref64
import ref_avepool64
from fcn_object_detector_amd import lib as L

E_ARG, E_ALIGN = 1, 2
P = 0x10000      # any non-null, 16-byte aligned address
# dy, dx, N, H, W, C, dx_cstride, dx_coffset, k, stride, pad, OH, OW, dy_cstride, dy_coffset, accumulate
GOOD = dict(dy=P, dx=P, N=2, H=7, W=6, C=6, dx_cstride=12, dx_coffset=4, k=3, stride=2, pad=1, OH=4, OW=4, dy_cstride=8, dy_coffset=0, accumulate=0)


def call(**kw):
    a = dict(GOOD, **kw)
    return L.load().fcn_avepool_bwd_f32(*[a[k] for k in GOOD], None)


def test_symbol_and_prototype():
    lib = L.load()
    assert hasattr(lib, "fcn_avepool_bwd_f32") and "fcn_avepool_bwd_f32" in L.PROTOTYPES
    res, args = L.PROTOTYPES["fcn_avepool_bwd_f32"]
    mres, margs = L.PROTOTYPES["fcn_maxpool_bwd_f32"]
    assert res is mres and args == margs[:1] + margs[2:]      # the argument list of fcn_maxpool_bwd_f32 minus idx
    assert lib.fcn_abi_version() == 2


def test_the_sample_geometry_is_a_valid_one():
    assert (GOOD["OH"], GOOD["OW"]) == (ref64.pool_out(7, 3, 1, 2), ref64.pool_out(6, 3, 1, 2))


@pytest.mark.parametrize("bad", [dict(dy=None), dict(dx=None), dict(N=0), dict(H=0), dict(W=-1), dict(C=0), dict(k=0), dict(stride=0),
                                 dict(pad=-1), dict(OH=0), dict(OW=0), dict(OH=6), dict(OW=5), dict(dx_coffset=-4), dict(dy_coffset=-4),
                                 dict(dx_cstride=8), dict(dy_cstride=4), dict(dy_coffset=4)])
def test_bad_arguments(bad):
    assert call(**bad) == E_ARG, bad
    assert b"avepool_bwd" in L.load().fcn_last_error_string()


@pytest.mark.parametrize("bad", [dict(dx_cstride=13), dict(dx_coffset=2), dict(dy_cstride=9), dict(dy_coffset=1, dy_cstride=12),
                                 dict(dy=P + 4), dict(dx=P + 8)])
def test_misaligned_arguments(bad):
    assert call(**bad) == E_ALIGN, bad
    assert b"avepool_bwd" in L.load().fcn_last_error_string()


@pytest.mark.parametrize("k,s,p,h,w", ref_avepool64.CASES)
def test_reference_against_torch_autograd(k, s, p, h, w):
    import torch
    import torch.nn.functional as F
    rng = np.random.default_rng(5)
    x = torch.tensor(rng.standard_normal((2, 3, h, w)), dtype=torch.float64, requires_grad=True)
    y = F.avg_pool2d(x, k, s, p, ceil_mode=True, count_include_pad=True)
    assert tuple(y.shape[2:]) == (ref64.pool_out(h, k, p, s), ref64.pool_out(w, k, p, s))
    np.testing.assert_allclose(y.detach().numpy(), ref64.ave_pool(x.detach().numpy(), k, s, p), rtol=1e-13, atol=1e-14)
    dy = rng.standard_normal(tuple(y.shape))
    y.backward(torch.tensor(dy))
    got = ref_avepool64.ave_pool_bwd(dy, k, s, p, h, w)
    np.testing.assert_allclose(got, x.grad.numpy(), rtol=1e-13, atol=1e-14)
    cnt = ref_avepool64.cover_count(k, s, p, h, w)
    assert np.all(got[:, :, cnt == 0] == 0)
    if s > k:
        assert (cnt == 0).any()
