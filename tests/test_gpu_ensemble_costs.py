"""jh_ensemble_costs through the C ABI: the mean of the `worst` largest of a rollout's M member costs, bit for bit against its numpy restatement
(judo_amd.ensemble.aggregate_costs_host), with ties, +inf and the 3.0e38 sentinel among the inputs; and its refusals."""

import numpy as np
import pytest

from tests.test_gpu_plan_batch import _err

pytestmark = pytest.mark.gpu


def _inputs(M, N, ld, seed):
    """(M, ld) fp32 member costs with deliberate ties: member 1 repeats member 0, member 2 is quantised to a handful of values (ties within the row and, for small values
    of it, across rows), and a few entries are +inf or the 3.0e38 sentinel -- alone in their rollout, twice in it, and in every member of it."""
    rng = np.random.default_rng(seed)
    c = rng.uniform(0.5, 40.0, size=(M, ld)).astype(np.float32)
    if M >= 2:
        c[1] = c[0]
    if M >= 3:
        c[2] = np.round(c[2] / 8.0) * 8.0
        c[0, ::7] = c[2, ::7]
    for col, val, rows in ((3, np.inf, (0,)), (5, 3.0e38, (0,)), (11, 3.0e38, (0, M - 1)), (17, np.inf, (0, M - 1)), (23, 3.0e38, range(M)), (29, np.inf, range(M))):
        if col < N:
            for r in rows:
                c[r, col] = val
    return c


@pytest.mark.parametrize("N", [1, 255, 257, 300])
@pytest.mark.parametrize("M", [1, 2, 5, 32])
def test_ensemble_costs_equal_the_numpy_restatement(gpu, M, N):
    import torch

    from judo_amd import _lib
    from judo_amd.ensemble import aggregate_costs_host

    L = _lib.lib()
    ld = N + 4
    c = _inputs(M, N, ld, seed=100 * M + N)
    d_c = torch.from_numpy(c).to(gpu)
    for worst in sorted({j for j in (1, 2, M) if j <= M}):
        out = torch.full((ld,), -7.0, dtype=torch.float32, device=gpu)
        _lib.check(L.jh_ensemble_costs(d_c.data_ptr(), M, N, ld, worst, out.data_ptr(), 0), "jh_ensemble_costs")
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        want = aggregate_costs_host(c[:, :N], worst)
        np.testing.assert_array_equal(got[:N].view(np.uint32), want.view(np.uint32), err_msg=f"M={M} N={N} worst={worst}")
        assert (got[N:] == -7.0).all(), "the floats between N and ld were written"
        if N > 29 and M > 1:
            assert got[29] == np.inf and got[3] == np.inf and (got[23] == np.inf) == (worst > 1)
    assert d_c.cpu().numpy().tobytes() == c.tobytes()  # the inputs are read only


def test_ensemble_costs_refusals(gpu):
    import torch

    from judo_amd import _lib

    L = _lib.lib()
    c = torch.ones((33, 12), dtype=torch.float32, device=gpu)
    out = torch.zeros(12, dtype=torch.float32, device=gpu)

    def call(M=4, N=8, ld=12, worst=2, mc=c.data_ptr(), o=out.data_ptr()):
        return L.jh_ensemble_costs(mc, M, N, ld, worst, o, 0)

    assert call() == 0
    assert call(M=0) == -1 and "M = 0" in _err()
    assert call(M=33) == -1 and "M = 33" in _err() and "JH_MAX_ENSEMBLE" in _err()
    assert call(worst=0) == -1 and "worst = 0" in _err()
    assert call(worst=5) == -1 and "worst = 5" in _err() and "M = 4" in _err()
    assert call(mc=None) == -1 and "member_costs" in _err() and "null" in _err()
    assert call(o=None) == -1 and "costs is a null" in _err()
    assert call(N=0) == -1 and "N must be positive" in _err()
    assert call(ld=7) == -1 and "ld (7) < N (8)" in _err()
    torch.cuda.synchronize()
