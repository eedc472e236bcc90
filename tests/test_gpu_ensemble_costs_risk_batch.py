"""jh_ensemble_costs_risk_batch through the C ABI: B controllers' member costs aggregated in one launch, each under the risk record it names -- the counted measure
where the tail word is 0.0, the plant-weighted tail mean under the M weights behind it otherwise -- bit for bit against the numpy restatement
(judo_amd.ensemble.aggregate_costs_risk_batch_host, which tests/test_weighted_fleet_host.py holds to the header's properties on the CPU).

One launch mixes the measures: controller 0 counted with `worst` = 2, controller 1 one-hot weights with tail 1 (its result is that member's row exactly), controller 2
general weights with tail 0.3 and 2^-20 on inputs with a three-way tie and a +inf member of weight zero.  NaN stands between N and ld and behind the 1 + M words of a
record; the words between N and ldc are found untouched.  No tolerance appears in this file."""

import ctypes as C

import numpy as np
import pytest

from tests.test_gpu_plan_batch import _err

pytestmark = pytest.mark.gpu

B = 3
PAD_LD, PAD_LDC, PAD_REC = 5, 3, 2


def _ints(*v):
    return (C.c_int * len(v))(*v)


def _inputs(M, N, seed):
    """(B, M, ld) member costs of both signs with NaN between N and ld, `worst` and the (B, 1 + M + PAD_REC) records with NaN behind 1 + M.  Controller 2: members 1 and
    2 repeat member 0 in the rollouts 3, 9, 15 ... (a three-way tie, M >= 3), and the last member has weight zero and is +inf in every even rollout (M >= 2)."""
    rng = np.random.default_rng(seed)
    ld = N + PAD_LD
    c = (rng.standard_normal((B, M, ld)) * 10).astype(np.float32)
    p = rng.uniform(0.05, 1.0, M)
    if M >= 3:
        c[2, 1, 3::6] = c[2, 0, 3::6]
        c[2, 2, 3::6] = c[2, 0, 3::6]
    if M >= 2:
        p[M - 1] = 0.0
        c[2, M - 1, ::2] = np.inf
    c[:, :, N:] = np.nan
    risk = np.full((B, 1 + M + PAD_REC), np.nan, dtype=np.float32)
    risk[0, : 1 + M] = 0.0  # the counted measure
    risk[0, 1 : 1 + M] = np.nan  # ... whose weights are not read
    hot = np.zeros(M, np.float32)
    hot[M // 2] = 1.0
    risk[1, 0], risk[1, 1 : 1 + M] = 1.0, hot
    risk[2, 0], risk[2, 1 : 1 + M] = 0.3, (p / p.sum()).astype(np.float32)
    return c, [min(2, M), 1, M], risk


def _call(L, d_c, M, N, d_risk, worst, d_out):
    return L.jh_ensemble_costs_risk_batch(d_c.data_ptr(), B, M, N, N + PAD_LD, d_risk.data_ptr(), 1 + M + PAD_REC, _ints(*worst), d_out.data_ptr(), N + PAD_LDC, 0)


@pytest.mark.parametrize("N", [1, 255, 257])
@pytest.mark.parametrize("M", [1, 3, 32])
def test_mixed_records_equal_the_numpy_restatement(gpu, M, N):
    import torch

    from judo_amd import _lib
    from judo_amd.ensemble import aggregate_costs_risk_batch_host

    L = _lib.lib()
    c, worst, risk = _inputs(M, N, seed=1000 * M + N)
    d_c = torch.from_numpy(c).to(gpu)
    for tail2 in (0.3, 2.0**-20):
        risk[2, 0] = tail2
        d_risk = torch.from_numpy(risk).to(gpu)
        out = torch.full((B, N + PAD_LDC), -7.0, dtype=torch.float32, device=gpu)
        _lib.check(_call(L, d_c, M, N, d_risk, worst, out), "jh_ensemble_costs_risk_batch")
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        with np.errstate(invalid="ignore"):
            clean = np.nan_to_num(risk[:, : 1 + M], nan=0.0)  # (controller 0's unread weights: the restatement does not read them either, but takes no NaN array apart)
        want = aggregate_costs_risk_batch_host(c[:, :, :N], worst, clean)
        np.testing.assert_array_equal(got[:, :N].view(np.uint32), want.view(np.uint32), err_msg=f"M={M} N={N} tail={tail2}")
        assert (got[:, N:] == -7.0).all(), "the floats between N and ldc were written"
        assert got[1, :N].tobytes() == c[1, M // 2, :N].tobytes()  # one-hot, tail 1: the member's row
        assert np.isfinite(got[2, :N]).all()  # the +inf member has weight zero: no inf, no NaN
        assert d_risk.cpu().numpy().tobytes() == risk.tobytes() and d_c.cpu().numpy().tobytes() == c.tobytes()  # the inputs are read only


@pytest.mark.parametrize("M,N", [(1, 1), (3, 257), (32, 255)])
def test_all_tail_words_zero_is_jh_ensemble_costs_per_controller(gpu, M, N):
    import torch

    from judo_amd import _lib

    L = _lib.lib()
    c, _, risk = _inputs(M, N, seed=7 * M + N)
    c[2][np.isinf(c[2])] = 3.0e38  # (the counted measure adds what it takes: the sentinel, and 3.0e38 + 3.0e38 = +inf as IEEE makes it)
    worst = [1, M, (M + 1) // 2]
    risk[:, 0] = 0.0
    d_c, d_risk = torch.from_numpy(c).to(gpu), torch.from_numpy(risk).to(gpu)
    out = torch.full((B, N + PAD_LDC), -7.0, dtype=torch.float32, device=gpu)
    _lib.check(_call(L, d_c, M, N, d_risk, worst, out), "jh_ensemble_costs_risk_batch")
    one = torch.full((B, N), -7.0, dtype=torch.float32, device=gpu)
    for b in range(B):
        _lib.check(L.jh_ensemble_costs(d_c[b].data_ptr(), M, N, N + PAD_LD, worst[b], one[b].data_ptr(), 0), "jh_ensemble_costs")
    torch.cuda.synchronize()
    assert out.cpu().numpy()[:, :N].tobytes() == one.cpu().numpy().tobytes()


def test_refusals(gpu):
    import torch

    from judo_amd import _lib

    L = _lib.lib()
    M, N = 4, 8
    c = torch.ones((B, M, 12), dtype=torch.float32, device=gpu)
    risk = torch.zeros((B, 1 + M), dtype=torch.float32, device=gpu)
    out = torch.full((B, 12), -7.0, dtype=torch.float32, device=gpu)
    base = dict(member_costs=c.data_ptr(), B=B, M=M, N=N, ld=12, risk=risk.data_ptr(), risk_stride_floats=1 + M, worst=_ints(1, 2, 4), costs=out.data_ptr(), ldc=12, stream=0)

    def call(**kw):
        return L.jh_ensemble_costs_risk_batch(*{**base, **kw}.values())

    for ptr in ("member_costs", "risk", "worst", "costs"):
        assert call(**{ptr: None}) == -1 and f"ensemble_costs_risk_batch: {ptr} is a null pointer" in _err(), ptr
    assert call(B=0) == -1 and "B = 0" in _err()
    assert call(B=257, worst=_ints(*([1] * 257))) == -1 and "B = 257" in _err() and "JH_MAX_ENSEMBLE_FLEET = 256" in _err()
    assert call(M=0) == -1 and "M = 0" in _err()
    assert call(M=33) == -1 and "M = 33" in _err() and "JH_MAX_ENSEMBLE = 32" in _err()
    assert call(N=0) == -1 and "N must be positive" in _err()
    assert call(ld=7) == -1 and "ld (7) < N (8)" in _err()
    assert call(ldc=7) == -1 and "ldc (7) < N (8)" in _err()
    assert call(risk_stride_floats=M) == -1 and "risk_stride_floats = 4" in _err() and "1 + M = 5" in _err()
    assert call(worst=_ints(1, 0, 4)) == -1 and "controller 1" in _err() and "worst = 0" in _err()
    assert call(worst=_ints(1, 2, 5)) == -1 and "controller 2" in _err() and "worst = 5" in _err() and "M = 4" in _err()
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == -7.0).all()  # nothing ran
    assert call() == 0
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert (got[:, :N] == 1.0).all() and (got[:, N:] == -7.0).all()
