"""jh_ensemble_costs_weighted through the C ABI: the tail mean of a rollout's M member costs under plant weights, bit for bit against its numpy restatement
(judo_amd.ensemble.aggregate_costs_weighted_host) with three-way ties, zero weights on +inf and 3.0e38 members and NaN between N and ld; bit for bit
jh_ensemble_costs where the two measures coincide; and its refusals."""

import ctypes

import numpy as np
import pytest

from tests.test_gpu_plan_batch import _err

pytestmark = pytest.mark.gpu

TAILS = (1.0, 0.5, 0.1, 2.0**-20)


def _floats(values):
    return (ctypes.c_float * len(values))(*[float(v) for v in values])


def _inputs(M, N, ld, seed):
    """(M, ld) fp32 member costs of both signs, NaN between N and ld, and fp32 weights.  Member 1 repeats member 0 in every third rollout and member 2 in every sixth
    (two-way and three-way ties); the last member has weight zero and carries +inf and the 3.0e38 sentinel (M > 1); with M >= 5 member 3 has weight zero too and ties
    with member 0 in places, and a positive-weight member carries a sentinel and a +inf that reach the tail."""
    rng = np.random.default_rng(seed)
    c = (rng.standard_normal((M, ld)) * 10).astype(np.float32)
    p = rng.uniform(0.05, 1.0, M)
    if M >= 2:
        c[1, ::3] = c[0, ::3]
    if M >= 3:
        c[2, ::6] = c[0, ::6]
    if M >= 2:
        p[M - 1] = 0.0
        c[M - 1, ::2] = np.inf
        c[M - 1, 1::4] = 3.0e38
    if M >= 5:
        p[3] = 0.0
        c[3, ::5] = c[0, ::5]
        c[0, 7::16] = 3.0e38
        c[1, 9::16] = np.inf
    c[:, N:] = np.nan
    return c, (p / p.sum()).astype(np.float32)


@pytest.mark.parametrize("N", [1, 64, 257])
@pytest.mark.parametrize("M", [1, 2, 3, 5, 32])
def test_weighted_costs_equal_the_numpy_restatement(gpu, M, N):
    import torch

    from judo_amd import _lib
    from judo_amd.ensemble import aggregate_costs_weighted_host

    L = _lib.lib()
    ld = N + 5
    c, p = _inputs(M, N, ld, seed=100 * M + N)
    d_c = torch.from_numpy(c).to(gpu)
    one_hot = np.zeros(M, np.float32)
    one_hot[M // 2] = 1.0
    for weights, tails in ((p, TAILS), (one_hot, (1.0,)), (p * np.float32(0.25), (1.0, 0.5))):  # (the last: weights that add up to less than the tail)
        for tail in tails:
            out = torch.full((ld,), -7.0, dtype=torch.float32, device=gpu)
            _lib.check(L.jh_ensemble_costs_weighted(d_c.data_ptr(), M, N, ld, _floats(weights), tail, out.data_ptr(), 0), "jh_ensemble_costs_weighted")
            torch.cuda.synchronize()
            got = out.cpu().numpy()
            want = aggregate_costs_weighted_host(c[:, :N], weights, tail)
            np.testing.assert_array_equal(got[:N].view(np.uint32), want.view(np.uint32), err_msg=f"M={M} N={N} tail={tail}")
            assert (got[N:] == -7.0).all(), "the floats between N and ld were written"
            if weights is one_hot:
                assert got[:N].tobytes() == c[M // 2, :N].tobytes()
            elif M in (2, 3):
                assert np.isfinite(got[:N]).all()  # the +inf and 3.0e38 members have weight zero: no inf, no NaN
    assert d_c.cpu().numpy().tobytes() == c.tobytes()  # the inputs are read only


def test_uniform_weights_are_the_worst_measure_on_distinct_costs(gpu):
    """M = 8, weights 1 / 8, tail j / 8 on pairwise-distinct costs: bit for bit jh_ensemble_costs(worst = j)."""
    import torch

    from judo_amd import _lib

    L = _lib.lib()
    M, N = 8, 300
    c = (np.random.default_rng(8).standard_normal((M, N)) * 7).astype(np.float32)
    assert all(len(set(col.tolist())) == M for col in c.T)
    d_c = torch.from_numpy(c).to(gpu)
    got, want = (torch.zeros(N, dtype=torch.float32, device=gpu) for _ in range(2))
    for j in range(1, M + 1):
        _lib.check(L.jh_ensemble_costs_weighted(d_c.data_ptr(), M, N, N, _floats([1.0 / M] * M), j / M, got.data_ptr(), 0), "jh_ensemble_costs_weighted")
        _lib.check(L.jh_ensemble_costs(d_c.data_ptr(), M, N, N, j, want.data_ptr(), 0), "jh_ensemble_costs")
        torch.cuda.synchronize()
        assert got.cpu().numpy().tobytes() == want.cpu().numpy().tobytes(), j


def test_weighted_costs_refusals(gpu):
    import torch

    from judo_amd import _lib

    L = _lib.lib()
    c = torch.ones((33, 12), dtype=torch.float32, device=gpu)
    out = torch.full((12,), -7.0, dtype=torch.float32, device=gpu)

    def call(M=4, N=8, ld=12, w=(0.25, 0.25, 0.5, 0.0), tail=0.5, mc=c.data_ptr(), o=out.data_ptr()):
        return L.jh_ensemble_costs_weighted(mc, M, N, ld, None if w is None else _floats(w), tail, o, 0)

    assert call(M=0, w=(1.0,)) == -1 and "M = 0" in _err()
    assert call(M=33, w=[1.0] * 33) == -1 and "M = 33" in _err() and "JH_MAX_ENSEMBLE" in _err()
    assert call(mc=None) == -1 and "member_costs" in _err() and "null" in _err()
    assert call(o=None) == -1 and "costs is a null" in _err()
    assert call(N=0) == -1 and "N must be positive" in _err()
    assert call(ld=7) == -1 and "ld (7) < N (8)" in _err()
    assert call(w=None) == -1 and "weights is a null pointer" in _err()
    assert call(w=(0.5, -0.25, 0.5, 0.25)) == -1 and "weights[1] = -0.25" in _err() and "negative or not finite" in _err()
    assert call(w=(0.5, 0.25, 0.5, float("nan"))) == -1 and "weights[3]" in _err() and "not finite" in _err()
    assert call(w=(float("inf"), 0.25, 0.5, 0.1)) == -1 and "weights[0]" in _err()
    assert call(w=(0.0, 0.0, 0.0, 0.0)) == -1 and "weights are all zero" in _err()
    for tail in (0.0, -0.5, 1.5, float("nan")):
        assert call(tail=tail) == -1 and "tail = " in _err() and "outside (0, 1]" in _err(), tail
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == -7.0).all()  # nothing ran
    assert call() == 0
    assert call(w=(0.0, 0.0, 0.0, 1e-30), tail=1.0) == 0  # one positive weight is enough, and the weights need not add up to 1
    torch.cuda.synchronize()
    assert (out.cpu().numpy()[:8] == 1.0).all()
