"""judo_amd.identify without a device: the numpy restatement of jh_plant_residuals against a plain fp64 evaluation and on known answers, the posterior arithmetic against
hand-computed values, the recording (ring buffer, chained steps, gaps), the hand-over to an `Assignment`, and every refusal.

The estimator is made on a stand-in for a `GpuModelSet` whose members live on the CPU device: everything up to the launch is host work and torch tensors.  Where a test
needs errors, it gives the estimator's `_score` (the launch and the kernel, tests/test_gpu_plant_estimator.py) fixed values."""

from types import SimpleNamespace

import numpy as np
import pytest


def _host_set(task="cartpole", M=3):
    """What a PlantEstimator reads of a GpuModelSet, on the CPU device."""
    import torch

    from judo_amd.models import layout, load_description

    desc = load_description(task)
    lay = layout(desc)
    model = SimpleNamespace(desc=desc, nq=lay.nq, nx=lay.nq + lay.nv, nu=lay.nu, device=torch.device("cpu"))
    return SimpleNamespace(models=[model] * M)


def _estimator(errors=None, task="cartpole", M=3, **kw):
    from judo_amd.identify import PlantEstimator

    est = PlantEstimator(_host_set(task, M), **kw)
    if errors is not None:
        est._score = lambda: np.asarray(errors, dtype=np.float32)[:, -len(est):]
    return est


def _window(est, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal(est.nx), rng.standard_normal((est.horizon, est.nu)), rng.standard_normal((est.horizon, est.nx))


def _unit_quats(rng, shape):
    q = rng.standard_normal(shape + (4,))
    return q / np.linalg.norm(q, axis=-1, keepdims=True)


def _residuals_fp64(pred, obs, weight, quat_adr):
    """The plain evaluation: fp64 throughout, the sum in numpy's own order."""
    W, H, nx = obs.shape
    p = np.asarray(pred, dtype=np.float64).reshape(-1, W, H, nx)
    o = np.broadcast_to(np.asarray(obs, dtype=np.float64), p.shape).copy()
    for a in quat_adr:
        flip = (p[..., a : a + 4] * o[..., a : a + 4]).sum(-1) < 0
        o[..., a : a + 4] = np.where(flip[..., None], -o[..., a : a + 4], o[..., a : a + 4])
    return (np.asarray(weight, dtype=np.float64) * (p - o) ** 2).sum(axis=(-1, -2))


def test_header_table_and_library_agree_on_the_entry():
    import ctypes
    import os
    import re

    from judo_amd import _lib, identify
    from tests.conftest import ROOT

    header = open(os.path.join(ROOT, "include", "judo_amd.h")).read()
    for name, val in (("JH_MAX_ID_HORIZON", _lib.MAX_ID_HORIZON), ("JH_MAX_ID_QUATS", _lib.MAX_ID_QUATS)):
        m = re.search(rf"#define\s+{name}\s+(\d+)", header)
        assert m and int(m.group(1)) == val, name
    assert (identify.MAX_ID_HORIZON, identify.MAX_ID_QUATS) == (64, 4)
    m = re.search(r"\bint\s+jh_plant_residuals\s*\(([^;]*)\)\s*;", header)
    assert m, "jh_plant_residuals is not declared"
    params = [re.findall(r"[A-Za-z_0-9]+", p)[-1] for p in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",")]
    assert params == ["pred", "obs", "weight", "quat_adr", "nquat", "M", "W", "H", "nx", "nq", "err", "ld", "stream"]
    res, args = _lib._SIGNATURES["jh_plant_residuals"]
    assert res is ctypes.c_int and len(args) == len(params) and args[3] == ctypes.POINTER(ctypes.c_int)
    assert "jh_plant_residuals" in _lib.EXPORTED_SYMBOLS and hasattr(ctypes.CDLL(_lib.LIB_PATH), "jh_plant_residuals")


# ---- the restatement ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,W,H,nx,quats", [(3, 5, 3, 4, ()), (2, 3, 7, 45, (3,)), (1, 1, 1, 6, ()), (4, 2, 64, 13, (3, 7)), (2, 65, 8, 31, (10,))])
def test_restatement_agrees_with_fp64(M, W, H, nx, quats):
    """Every term is non-negative, so the rounding errors only add up: a subtraction, two products, nx - 1 step adds and six halvings per term give a relative error of
    at most (nx + 8) * 2**-24 to first order -- the bound the operation count gives."""
    from judo_amd.identify import plant_residuals_host

    rng = np.random.default_rng(M * 1000 + W * 10 + H)
    obs = rng.standard_normal((W, H, nx))
    pred = obs[None] + 0.3 * rng.standard_normal((M, W, H, nx))
    for a in quats:  # unit quaternions, the predictions near the observation or near its antipode: the dot product is far from 0 and its sign the same in both precisions
        obs[..., a : a + 4] = _unit_quats(rng, (W, H))
        sign = rng.choice([-1.0, 1.0], size=(M, W, H, 1))
        q = sign * obs[None, ..., a : a + 4] + 0.05 * rng.standard_normal((M, W, H, 4))
        pred[..., a : a + 4] = q / np.linalg.norm(q, axis=-1, keepdims=True)
    obs, pred = obs.astype(np.float32), pred.astype(np.float32).reshape(M * W, H, nx)
    weight = rng.uniform(0.5, 4.0, nx).astype(np.float32)
    got = plant_residuals_host(pred, obs, weight, quats, nq=nx)
    want = _residuals_fp64(pred, obs, weight, quats)
    assert got.dtype == np.float32 and got.shape == (M, W) and (want > 0).all()
    rel = float(np.max(np.abs(got.astype(np.float64) - want) / want))
    print(f"M={M} W={W} H={H} nx={nx}: largest relative error {rel:.3e}, bound {(nx + 8) * 2.0**-24:.3e}")
    assert rel <= (nx + 8) * 2.0**-24


@pytest.mark.parametrize("H", [1, 3, 7, 64])
def test_known_answers(H):
    from judo_amd.identify import plant_residuals_host

    rng = np.random.default_rng(H)
    M, W, nx, a = 2, 3, 9, 3
    obs = rng.standard_normal((W, H, nx)).astype(np.float32)
    obs[..., a : a + 4] = _unit_quats(rng, (W, H)).astype(np.float32)
    weight = rng.uniform(0.5, 2.0, nx).astype(np.float32)
    same = np.tile(obs, (M, 1, 1))
    zero = np.zeros((M, W), dtype=np.float32)
    assert np.array_equal(plant_residuals_host(same, obs, weight, (a,), nq=7), zero)  # pred == obs
    anti = same.copy()
    anti[W:, :, a : a + 4] *= -1  # plant 1 predicts the antipodal quaternion in every row: the same pose
    assert np.array_equal(plant_residuals_host(anti, obs, weight, (a,), nq=7), zero)
    assert (plant_residuals_host(anti, obs, weight, (), nq=7)[1] > 0).all()  # ... which only the alignment tells
    off = same.copy()
    off[..., 8] += 0.5
    w0 = weight.copy()
    w0[8] = 0.0  # a zero weight removes its coordinate
    assert np.array_equal(plant_residuals_host(off, obs, w0, (a,), nq=7), zero)
    got = plant_residuals_host(off, obs, weight, (a,), nq=7)
    assert (got > 0).all()
    # one coordinate off in every step: the halving adds the H step sums s_h in its own order
    e = off[0, :, 8] - obs[0, :, 8]
    s = (weight[8] * e) * e
    want = {1: lambda: s[0], 3: lambda: (s[0] + s[2]) + s[1], 7: lambda: ((s[0] + s[4]) + (s[2] + s[6])) + ((s[1] + s[5]) + s[3])}.get(H)
    if want is not None:
        assert s.dtype == np.float32 and got[0, 0] == want()


def test_restatement_refusals():
    from judo_amd.identify import plant_residuals_host

    obs, w = np.zeros((2, 3, 8), np.float32), np.ones(8, np.float32)
    pred = np.zeros((4, 3, 8), np.float32)
    assert plant_residuals_host(pred, obs, w, (3,), nq=7).shape == (2, 2)
    for kw, text in ((dict(pred=pred[:3]), "pred must be"), (dict(weight=w[:5]), "weight must have nx = 8"), (dict(nq=9), "nq = 9"), (dict(quat_adr=(4,), nq=7), r"quat_adr\[0\] = 4"),
                     (dict(quat_adr=(-1,)), r"quat_adr\[0\] = -1"), (dict(quat_adr=(0, 3)), r"quat_adr\[1\] = 3 overlaps quat_adr\[0\] = 0"),
                     (dict(quat_adr=(0, 4, 0, 4, 0)), "nquat = 5"), (dict(obs=np.zeros((2, 65, 8), np.float32)), "JH_MAX_ID_HORIZON")):
        args = {**dict(pred=pred, obs=obs, weight=w, quat_adr=(), nq=None), **kw}
        with pytest.raises(ValueError, match=text):
            plant_residuals_host(**args)


# ---- the posterior -----------------------------------------------------------------------------------------------------------------------------------------------
ERRORS = [[2.0, 4.0], [0.0, 0.0], [6.0, 2.0]]  # (M = 3, two windows, the older first)


def _fill(est, n):
    for i in range(n):
        est.observe(*_window(est, i))


def test_posterior_hand_computed():
    est = _estimator(ERRORS, horizon=2, windows=4)
    assert len(est) == 0 and np.array_equal(est.update(), np.full(3, 1 / 3)) and est.errors.shape == (3, 0) and not est.degenerate  # no window: the prior
    _fill(est, 2)
    z = np.array([np.exp(-3.0), 1.0, np.exp(-4.0)])  # L = 0.5 * (2 + 4), 0, 0.5 * (6 + 2)
    np.testing.assert_allclose(est.update(), z / z.sum(), rtol=1e-14)
    np.testing.assert_allclose(est.log_likelihood, [-3.0, 0.0, -4.0], rtol=1e-14)
    assert est.map == 1 and not est.degenerate and est.errors.shape == (3, 2) and est.errors.dtype == np.float32

    est = _estimator(ERRORS, horizon=2, windows=4, prior=[2.0, 1.0, 1.0])  # the prior, normalised
    _fill(est, 2)
    z = np.array([0.5 * np.exp(-3.0), 0.25, 0.25 * np.exp(-4.0)])
    np.testing.assert_allclose(est.update(), z / z.sum(), rtol=1e-14)

    est = _estimator(ERRORS, horizon=2, windows=4, temperature=2.0)  # the temperature divides L
    _fill(est, 2)
    z = np.array([np.exp(-1.5), 1.0, np.exp(-2.0)])
    np.testing.assert_allclose(est.update(), z / z.sum(), rtol=1e-14)

    est = _estimator(ERRORS, horizon=2, windows=4, discount=0.5)  # the older window, age 1, counts half
    _fill(est, 2)
    z = np.array([np.exp(-2.5), 1.0, np.exp(-2.5)])
    np.testing.assert_allclose(est.update(), z / z.sum(), rtol=1e-14)
    np.testing.assert_allclose(est.log_likelihood, [-0.5 * (0.5 * 2 + 4), 0.0, -0.5 * (0.5 * 6 + 2)], rtol=1e-14)

    est = _estimator([[2.0, np.nan], [0.0, 0.0], [6.0, 2.0]], horizon=2, windows=4)  # a non-finite error counts as +inf: likelihood zero
    _fill(est, 2)
    z = np.array([0.0, 1.0, np.exp(-4.0)])
    np.testing.assert_allclose(est.update(), z / z.sum(), rtol=1e-14)
    assert est.update()[0] == 0.0 and est.log_likelihood[0] == -np.inf and not est.degenerate

    est = _estimator([[np.inf, 1.0], [np.nan, 0.0], [6.0, -np.inf]], horizon=2, windows=4, prior=[0.2, 0.3, 0.5])  # all infinite: the prior, and it says so
    _fill(est, 2)
    np.testing.assert_allclose(est.update(), [0.2, 0.3, 0.5], rtol=1e-15)
    assert est.degenerate

    est = _estimator(ERRORS, horizon=2, windows=4, prior=[0.0, 0.0, 1.0])  # a zero prior stays zero
    _fill(est, 2)
    assert np.array_equal(est.update(), [0.0, 0.0, 1.0]) and not est.degenerate


def test_an_old_infinite_error_stays_infinite():
    """discount**age underflows to 0 for an old window; 0 * inf must not turn the plant's L into NaN."""
    from judo_amd.identify import posterior_from_errors

    e = np.zeros((2, 1200))
    e[0, 0] = np.inf
    post, ll, degenerate = posterior_from_errors(e, None, 1.0, 0.5)
    assert np.array_equal(post, [0.0, 1.0]) and ll[0] == -np.inf and not degenerate


# ---- the recording -----------------------------------------------------------------------------------------------------------------------------------------------
def test_ring_buffer_replaces_its_oldest_window():
    est = _estimator(horizon=2, windows=3)
    wins = [_window(est, i) for i in range(5)]
    for i, w in enumerate(wins):
        est.observe(*w)
        assert len(est) == min(i + 1, 3)
        x0, u, s = est.recorded()
        kept = wins[max(0, i - 2) : i + 1]  # the newest three, oldest first
        assert np.array_equal(x0, np.stack([k[0] for k in kept]).astype(np.float32))
        assert np.array_equal(u, np.stack([k[1] for k in kept]).astype(np.float32)) and np.array_equal(s, np.stack([k[2] for k in kept]).astype(np.float32))
    est.reset()
    assert len(est) == 0 and est.recorded()[0].shape == (0, est.nx)
    est.reset(prior=[1, 1, 2])
    assert np.array_equal(est.update(), [0.25, 0.25, 0.5])


def test_observe_step_chains_steps_and_detects_a_gap():
    est = _estimator(horizon=3, windows=4)
    rng = np.random.default_rng(0)
    xs, us = rng.standard_normal((9, est.nx)), rng.standard_normal((9, est.nu))
    for t in range(3):
        assert len(est) == 0 and est.pending_steps == t
        est.observe_step(xs[t], us[t], xs[t + 1])
    assert len(est) == 1 and est.pending_steps == 0
    x0, u, s = est.recorded()
    assert np.array_equal(x0[0], xs[0].astype(np.float32)) and np.array_equal(u[0], us[:3].astype(np.float32)) and np.array_equal(s[0], xs[1:4].astype(np.float32))
    est.observe_step(xs[3], us[3], xs[4])
    est.observe_step(xs[4], us[4], xs[5])
    assert est.pending_steps == 2
    gap = xs[5].copy()
    gap[1] = np.nextafter(gap[1], np.inf)  # one element off by one ulp: a gap in the recording
    est.observe_step(gap, us[5], xs[6])
    assert est.pending_steps == 1 and len(est) == 1  # the two pending steps are dropped, a new window starts at `gap`
    est.observe_step(xs[6], us[6], xs[7])
    est.observe_step(xs[7], us[7], xs[8])
    assert len(est) == 2 and est.pending_steps == 0
    x0, u, s = est.recorded()
    assert np.array_equal(x0[1], gap.astype(np.float32)) and np.array_equal(u[1], us[5:8].astype(np.float32)) and np.array_equal(s[1], xs[6:9].astype(np.float32))


# ---- the hand-over -----------------------------------------------------------------------------------------------------------------------------------------------
def _assignment_controller(M=3, blocks=8):
    from judo_amd.plants import Assignment

    class Ctrl(Assignment):
        def __init__(self):
            self._descriptions = [{}] * M
            self._init_assignment(blocks, None, M)

    return Ctrl()


def test_apply_hands_the_posterior_to_an_assignment():
    from judo_amd.plants import blocks_from_weights

    est = _estimator([[np.inf], [np.inf], [0.0]], horizon=2, windows=4)
    _fill(est, 1)
    ctrl = _assignment_controller()
    assert ctrl.assignment == [0, 1, 2, 0, 1, 2, 0, 1]
    w = est.apply(ctrl, floor=0.25)  # (the posterior is computed on demand: a window arrived since the last update)
    assert np.array_equal(est.posterior, [0.0, 0.0, 1.0])
    np.testing.assert_allclose(w, [1 / 12, 1 / 12, 10 / 12], rtol=1e-15)
    np.testing.assert_allclose(8 * w, [0.667, 0.667, 6.667], atol=5e-4)  # the quotas: a block each from the remainders, six and the largest remainder for plant 2
    assert ctrl.assignment == [0, 1, 2, 2, 2, 2, 2, 2] == blocks_from_weights(w, 8)
    est.apply(ctrl, floor=0.0)
    assert ctrl.assignment == [2] * 8
    est.apply(ctrl, floor=1.0)
    assert ctrl.assignment == [0, 0, 0, 1, 1, 1, 2, 2]


# ---- the refusals ------------------------------------------------------------------------------------------------------------------------------------------------
def test_estimator_refusals():
    from judo_amd.identify import PlantEstimator
    from judo_amd.plants import WorstCase
    from judo_amd.policy import SpotPlantSet

    spot = SpotPlantSet.__new__(SpotPlantSet)  # (no device: the refusal reads the type alone)
    with pytest.raises(ValueError, match="SpotPlantSet.*policy state"):
        PlantEstimator(spot)
    with pytest.raises(ValueError, match="SpotPlantSet"):
        PlantEstimator.for_controller(SimpleNamespace(plants=spot))
    with pytest.raises(ValueError, match="ctrl is a SimpleNamespace.*no GpuModelSet"):
        PlantEstimator.for_controller(SimpleNamespace())
    with pytest.raises(ValueError, match="model_set must be a GpuModelSet, got list"):
        PlantEstimator([1, 2])
    for kw, text in ((dict(horizon=0), "horizon = 0"), (dict(horizon=65), "horizon = 65.*JH_MAX_ID_HORIZON"), (dict(windows=0), "windows = 0"),
                     (dict(prior=[0.5, 0.5]), "prior has 2 entries for M = 3"), (dict(prior=[0.5, -0.1, 0.6]), "prior must be non-negative"), (dict(prior=[0, 0, 0]), "prior has zero sum"),
                     (dict(temperature=0.0), "temperature = 0.0"), (dict(temperature=-1.0), "temperature = -1.0"), (dict(discount=0.0), "discount = 0.0"),
                     (dict(discount=1.5), "discount = 1.5"), (dict(state_sigma=0.0), "state_sigma"), (dict(state_sigma=[1.0, 2.0]), "state_sigma"),
                     (dict(state_sigma=np.inf), "state_sigma")):
        with pytest.raises(ValueError, match=text):
            _estimator(**kw)
    est = _estimator(horizon=4, windows=2, state_sigma=[0.5, 1.0, 2.0, 4.0])
    assert np.array_equal(est.weight, np.array([4.0, 1.0, 0.25, 0.0625], dtype=np.float32)) and est.weight.dtype == np.float32 and est.quat_adr == []
    x0, u, s = _window(est, 0)
    for args, text in (((x0[:3], u, s), "x0 must be"), ((x0, u[:3], s), r"controls must be \(horizon, nu\) = \(4, 1\)"), ((x0, u, s[:, :3]), r"states must be \(horizon, nx\) = \(4, 4\)"),
                       ((x0, u, s[:3]), "states must be")):
        with pytest.raises(ValueError, match=text):
            est.observe(*args)
    with pytest.raises(ValueError, match="x and x_next must be"):
        est.observe_step(x0[:3], u[0], x0)
    with pytest.raises(ValueError, match="u must be"):
        est.observe_step(x0, u[:2, 0], x0)
    assert len(est) == 0 and est.pending_steps == 0
    ctrl = _assignment_controller()
    for floor in (-0.1, 1.1, np.nan):
        with pytest.raises(ValueError, match="floor = "):
            est.apply(ctrl, floor=floor)

    class Ensemble(WorstCase):
        pass

    with pytest.raises(ValueError, match="Ensemble, an ensemble controller.*plant-weighted risk measure is out of scope.*set_member"):
        est.apply(Ensemble())
    with pytest.raises(ValueError, match="ctrl is a SimpleNamespace.*RandomizedController"):
        est.apply(SimpleNamespace())
    with pytest.raises(ValueError, match="4 weights for M = 3|3 weights for M = 4"):
        _estimator(M=4).apply(ctrl)
    assert ctrl.assignment == [0, 1, 2, 0, 1, 2, 0, 1]  # nothing was handed over


def test_quaternion_offsets_come_from_the_free_joints():
    est = _estimator(task="leap_cube", M=2)
    assert est.quat_adr == [3] and est.nq == 23 and est.nx == 45
    assert _estimator(task="fr3_pick", M=2).quat_adr == [3]
