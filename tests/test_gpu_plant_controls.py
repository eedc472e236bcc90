"""jh_plant_controls through the C ABI: B splines at their plants' own clocks, against the numpy restatement (judo_amd.simulation.plant_controls_host), bit for bit.

B = 3, S = 5, K = 4 with nu = 1 (cartpole) and nu = 16 (leap): the three spline kinds, per-plant knot grids shifted against one another, step0 = 2 into a poisoned buffer
of ld_steps = 9 -- no word outside the range is written --, the clip on and off.  One larger case has three workgroups per plant, the last one ragged."""

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

INVALID = -1
POISON = -7.0


def _case(kind, B, S, K, nu, seed):
    """(W (B, S, K) fp32, knots (B, K, nu) fp32): plant b's grid starts 0.013 * b later and its clock stands somewhere else on it; queries in front of, on and behind
    the span."""
    from judo_amd.spline import spline_weights

    rng = np.random.default_rng(seed)
    dt = 0.01
    W = []
    for b in range(B):
        grid = 0.013 * b + np.linspace(0.0, dt * (S - 2), K)
        clock = grid[0] - dt + 0.004 * b if b != 1 else grid[0]  # plant 1 starts on a knot
        W.append(spline_weights(kind, grid, clock + dt * np.arange(S)))
    return np.stack(W).astype(np.float32), rng.standard_normal((B, K, nu)).astype(np.float32)


def _call(W, knots, lohi, B, S, K, nu, step0, ld_steps, controls, knot_stride=None):
    from judo_amd import _lib
    from judo_amd.device import current_stream_ptr

    return _lib.lib().jh_plant_controls(_lib.ptr(W), _lib.ptr(knots), K * nu if knot_stride is None else knot_stride, _lib.ptr(lohi), B, S, K, nu, step0, ld_steps,
                                        _lib.ptr(controls), current_stream_ptr())


def _check(gpu, kind, B, S, K, nu, step0, ld_steps, clip, seed):
    import torch

    from judo_amd.simulation import plant_controls_host

    W, knots = _case(kind, B, S, K, nu, seed)
    lohi = np.concatenate([np.full(nu, -0.5), np.full(nu, 0.5)]).astype(np.float32) if clip else None
    want = plant_controls_host(W, knots, lohi)
    if clip:
        raw = plant_controls_host(W, knots)
        assert (raw < -0.5).any() and (raw > 0.5).any() and ((raw > -0.5) & (raw < 0.5)).any(), "the case clips nothing, or everything"
    out = torch.full((B, ld_steps, nu), POISON, dtype=torch.float32, device=gpu)
    st = _call(torch.from_numpy(W).to(gpu), torch.from_numpy(knots).to(gpu), None if lohi is None else torch.from_numpy(lohi).to(gpu), B, S, K, nu, step0, ld_steps, out)
    assert st == 0
    got = out.cpu().numpy()
    np.testing.assert_array_equal(got[:, step0 : step0 + S].view(np.uint32), want.view(np.uint32), err_msg=f"{kind} nu={nu} clip={clip}")
    outside = np.delete(got, np.arange(step0, step0 + S), axis=1)
    assert outside.size == B * (ld_steps - S) * nu and (outside == POISON).all(), "a word outside steps step0 .. step0 + S - 1 was written"


@pytest.mark.parametrize("nu", [1, 16], ids=["cartpole_nu1", "leap_nu16"])
@pytest.mark.parametrize("kind", ["zero", "linear", "cubic"])
def test_controls_equal_the_restatement(gpu, kind, nu):
    for clip in (False, True):
        _check(gpu, kind, 3, 5, 4, nu, 2, 9, clip, seed=10 * nu + clip)


def test_three_workgroups_per_plant(gpu):
    """S * nu = 37 * 16 = 592 = 2 * 256 + 80: two full workgroups and a ragged third per plant, K = 7, the buffer exactly as long as the range."""
    _check(gpu, "cubic", 3, 37, 7, 16, 0, 37, True, seed=3)


def test_a_knot_stride_of_its_own(gpu):
    """Knots that lie in a larger record per plant: knot_stride floats apart."""
    import torch

    from judo_amd.simulation import plant_controls_host

    B, S, K, nu, stride = 3, 5, 4, 2, 11
    W, knots = _case("linear", B, S, K, nu, 5)
    rec = np.full((B, stride), 99.0, dtype=np.float32)
    rec[:, : K * nu] = knots.reshape(B, -1)
    out = torch.empty((B, S, nu), dtype=torch.float32, device=gpu)
    assert _call(torch.from_numpy(W).to(gpu), torch.from_numpy(rec).to(gpu), None, B, S, K, nu, 0, S, out, knot_stride=stride) == 0
    np.testing.assert_array_equal(out.cpu().numpy().view(np.uint32), plant_controls_host(W, knots).view(np.uint32))


def test_refusals_name_the_argument(gpu):
    import torch

    from judo_amd import _lib

    B, S, K, nu = 3, 5, 4, 2
    W, knots = (torch.zeros((B, S, K), device=gpu), torch.zeros((B, K, nu), device=gpu))
    out = torch.full((B, 9, nu), POISON, dtype=torch.float32, device=gpu)
    ok = dict(W=W, knots=knots, lohi=None, B=B, S=S, K=K, nu=nu, step0=2, ld_steps=9, controls=out)
    for change, word in ((dict(W=None), "W is a null pointer"), (dict(knots=None), "knots is a null pointer"), (dict(controls=None), "controls is a null pointer"),
                         (dict(B=0), "B = 0"), (dict(B=257), "JH_MAX_FLEET_PLANT_BLOCKS"), (dict(S=0), "S = 0"), (dict(K=0), "K = 0"), (dict(nu=0), "nu = 0"),
                         (dict(K=64, nu=9), "JH_MAX_KNOT_DIM"), (dict(knot_stride=7), "knot_stride = 7"), (dict(step0=-1), "step0 = -1"), (dict(ld_steps=6), r"ld_steps (6) < step0 + S")):
        assert _call(**{**ok, **change}) == INVALID, change
        msg = _lib.lib().jh_last_error().decode()
        assert word in msg and msg.startswith("plant_controls:"), (change, msg)
    torch.cuda.synchronize()
    assert (out == POISON).all()  # nothing was enqueued
