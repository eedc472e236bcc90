"""judo_amd.reports without a device: the numpy restatement of jh_plant_residuals_reports against a plain fp64 evaluation, against `plant_residuals_host` where the two
coincide, in both layouts and under the NaN rules; the recording of `ReportEstimator` (`observe`, `start`, `step`, `needs_start`, `reported`) and of
`SpotReportEstimator`, every refusal, and the hand-over to stand-in controllers.

The estimators are made on stand-ins whose members live on the CPU device, as in tests/test_plant_estimator_host.py: everything up to the launch is host work and torch
tensors.  Where a test needs errors, it gives the estimator's `_score` fixed values."""

import ctypes
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest


def _unit_quats(rng, shape):
    q = rng.standard_normal(shape + (4,))
    return q / np.linalg.norm(q, axis=-1, keepdims=True)


def _inputs(M, W, H, nx, ns, quats, seed):
    """(pred (M * W, H, nx), obs (W, H, nx), weight (nx), pred_sens, obs_sens, weight_sens) in fp32, plant-major: predictions around the observations, unit quaternions at
    the offsets, near the observed one or near its antipode -- the dot product is far from 0 and its sign the same in both precisions."""
    rng = np.random.default_rng(seed)
    obs = rng.standard_normal((W, H, nx))
    pred = obs[None] + 0.3 * rng.standard_normal((M, W, H, nx))
    for a in quats:
        obs[..., a : a + 4] = _unit_quats(rng, (W, H))
        sign = rng.choice([-1.0, 1.0], size=(M, W, H, 1))
        q = sign * obs[None, ..., a : a + 4] + 0.05 * rng.standard_normal((M, W, H, 4))
        pred[..., a : a + 4] = q / np.linalg.norm(q, axis=-1, keepdims=True)
    weight = rng.uniform(0.5, 4.0, nx)
    obs_sens = rng.standard_normal((W, H, ns))
    pred_sens = obs_sens[None] + 0.3 * rng.standard_normal((M, W, H, ns))
    f = np.float32
    sens = (pred_sens.reshape(M * W, H, ns).astype(f), obs_sens.astype(f), rng.uniform(0.5, 4.0, ns).astype(f)) if ns else (None, None, None)
    return (pred.reshape(M * W, H, nx).astype(f), obs.astype(f), weight.astype(f)) + sens


def _thin(obs, obs_sens, quats, seed):
    """NaN patterns on copies: every second step row, one column, one whole quaternion in some rows, scattered single readings (outside the quaternions), sensors too."""
    rng = np.random.default_rng(seed)
    o = obs.copy()
    W, H, nx = o.shape
    inq = np.zeros(nx, dtype=bool)
    for a in quats:
        inq[a : a + 4] = True
    o[:, 1::2] = np.nan
    free = np.flatnonzero(~inq)
    if free.size > 1:
        o[..., free[-1]] = np.nan
        o[..., free[:-1]] = np.where(rng.random((W, H, free.size - 1)) < 0.2, np.nan, o[..., free[:-1]])
    for a in quats[:1]:
        o[:, ::3, a : a + 4] = np.nan
    s = None
    if obs_sens is not None:
        s = np.where(rng.random(obs_sens.shape) < 0.4, np.float32(np.nan), obs_sens)
    return o, s


def _residuals_fp64(pred, obs, weight, quat_adr, pred_sens=None, obs_sens=None, weight_sens=None):
    """The plain evaluation of the rule: fp64 throughout, the sum in numpy's own order, an unreported entry contributing nothing."""
    W, H, nx = obs.shape
    p = np.asarray(pred, dtype=np.float64).reshape(-1, W, H, nx)
    o = np.broadcast_to(np.asarray(obs, dtype=np.float64), p.shape).copy()
    for a in quat_adr:
        with np.errstate(invalid="ignore"):
            flip = (p[..., a : a + 4] * o[..., a : a + 4]).sum(-1) < 0
        o[..., a : a + 4] = np.where(flip[..., None], -o[..., a : a + 4], o[..., a : a + 4])
    total = np.where(np.isnan(o), 0.0, np.asarray(weight, dtype=np.float64) * (p - o) ** 2).sum(axis=(-1, -2))
    if pred_sens is not None:
        ns = obs_sens.shape[-1]
        ps, os_ = np.asarray(pred_sens, dtype=np.float64).reshape(-1, W, H, ns), np.asarray(obs_sens, dtype=np.float64)
        total = total + np.where(np.isnan(os_), 0.0, np.asarray(weight_sens, dtype=np.float64) * (ps - os_) ** 2).sum(axis=(-1, -2))
    return total


def test_header_table_and_library_agree_on_the_entry():
    from judo_amd import _lib
    from tests.conftest import ROOT

    header = open(os.path.join(ROOT, "include", "judo_amd.h")).read()
    m = re.search(r"\bint\s+jh_plant_residuals_reports\s*\(([^;]*)\)\s*;", header)
    assert m, "jh_plant_residuals_reports is not declared"
    params = [re.findall(r"[A-Za-z_0-9]+", p)[-1] for p in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",")]
    assert params == ["pred", "obs", "weight", "quat_adr", "nquat", "pred_sens", "obs_sens", "weight_sens", "ns", "plant_stride", "window_stride", "M", "W", "H", "nx", "nq",
                      "err", "ld", "stream"]
    res, args = _lib._SIGNATURES["jh_plant_residuals_reports"]
    assert res is ctypes.c_int and len(args) == len(params) and args[3] == ctypes.POINTER(ctypes.c_int) and args[9] is ctypes.c_size_t and args[10] is ctypes.c_size_t
    assert "jh_plant_residuals_reports" in _lib.EXPORTED_SYMBOLS and hasattr(ctypes.CDLL(_lib.LIB_PATH), "jh_plant_residuals_reports")


# ---- the restatement ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H", [1, 3, 33, 64])
@pytest.mark.parametrize("ns", [0, 1, 5])
@pytest.mark.parametrize("nx", [1, 9])
def test_restatement_agrees_with_fp64(nx, ns, H):
    """Every term is non-negative, so the rounding errors only add up: per term a subtraction and two products, nx + ns - 1 step adds and six halvings give a relative
    error of at most (nx + ns + 8) * 2**-24 to first order -- the bound the operation count gives, full and thinned alike (a skipped term adds an exact +0.0)."""
    from judo_amd.reports import plant_residuals_reports_host

    M, W, quats = 3, 5, ((0, 4) if nx == 9 else ())
    pred, obs, weight, ps, os_, ws = _inputs(M, W, H, nx, ns, quats, seed=100 * nx + 10 * ns + H)
    bound = (nx + ns + 8) * 2.0**-24
    for thinned in (False, True):
        o, s = _thin(obs, os_, quats, seed=H) if thinned else (obs, os_)
        got = plant_residuals_reports_host(pred, o, weight, quats, nq=nx, pred_sens=ps, obs_sens=s, weight_sens=ws)
        want = _residuals_fp64(pred, o, weight, quats, ps, s, ws)
        assert got.dtype == np.float32 and got.shape == (M, W) and np.isfinite(got).all()
        assert (want > 0).all()  # (step 0 of every window is reported)
        rel = float(np.max(np.abs(got.astype(np.float64) - want) / want))
        print(f"nx={nx} ns={ns} H={H} thinned={thinned}: largest relative error {rel:.3e}, bound {bound:.3e}")
        assert rel <= bound


@pytest.mark.parametrize("M,W,H,nx,quats", [(3, 5, 3, 4, ()), (2, 3, 7, 45, (3,)), (1, 1, 1, 6, ()), (4, 2, 64, 13, (3, 7)), (3, 5, 33, 9, (0, 4))])
def test_restatement_is_plant_residuals_host_where_nothing_is_nan(M, W, H, nx, quats):
    from judo_amd.identify import plant_residuals_host
    from judo_amd.reports import plant_residuals_reports_host

    pred, obs, weight, *_ = _inputs(M, W, H, nx, 0, quats, seed=M + W + H)
    got, want = plant_residuals_reports_host(pred, obs, weight, quats, nq=nx), plant_residuals_host(pred, obs, weight, quats, nq=nx)
    assert got.view(np.uint32).tolist() == want.view(np.uint32).tolist() and (want > 0).all()


@pytest.mark.parametrize("ns", [0, 5])
def test_window_major_equals_plant_major_after_transposing(ns):
    from judo_amd.reports import plant_residuals_reports_host

    M, W, H, nx, quats = 3, 5, 7, 9, (0, 4)
    pred, obs, weight, ps, os_, ws = _inputs(M, W, H, nx, ns, quats, seed=5)
    obs, os_ = _thin(obs, os_, quats, seed=6)

    def t(a):  # row m * W + w -> row w * M + m
        return None if a is None else np.ascontiguousarray(a.reshape(M, W, H, -1).transpose(1, 0, 2, 3)).reshape(M * W, H, -1)

    pm = plant_residuals_reports_host(pred, obs, weight, quats, nq=nx, pred_sens=ps, obs_sens=os_, weight_sens=ws)
    wm = plant_residuals_reports_host(t(pred), obs, weight, quats, nq=nx, pred_sens=t(ps), obs_sens=os_, weight_sens=ws, window_major=True)
    assert pm.view(np.uint32).tolist() == wm.view(np.uint32).tolist() and (pm > 0).all()
    # (the transposition matters: read the other way, the rows belong to other pairs)
    assert not np.array_equal(pm, plant_residuals_reports_host(pred, obs, weight, quats, nq=nx, pred_sens=ps, obs_sens=os_, weight_sens=ws, window_major=True))


def test_nan_rules():
    from judo_amd.identify import plant_residuals_host
    from judo_amd.reports import plant_residuals_reports_host as host

    M, W, H, nx, ns, quats = 3, 4, 6, 9, 2, (0, 4)
    pred, obs, weight, ps, os_, ws = _inputs(M, W, H, nx, ns, quats, seed=17)
    full = host(pred, obs, weight, quats, nq=nx)
    p4 = pred.reshape(M, W, H, nx)

    # a row: step 2 of window 1 unreported is that step removed from the sum -- the other steps of that window scored alone, with the step's slot +0.0
    o = obs.copy()
    o[1, 2] = np.nan
    got = host(pred, o, weight, quats, nq=nx)
    assert np.array_equal(np.delete(got, 1, axis=1), np.delete(full, 1, axis=1)) and (got[:, 1] < full[:, 1]).all()
    same = pred.copy().reshape(M, W, H, nx)
    same[:, 1, 2] = obs[1, 2]  # a prediction equal to the observation in that row: the row's terms are exactly 0
    assert np.array_equal(got, plant_residuals_host(same.reshape(M * W, H, nx), obs, weight, quats, nq=nx))

    # a column: coordinate 8 unreported everywhere is weight 0 on it
    o = obs.copy()
    o[..., 8] = np.nan
    w0 = weight.copy()
    w0[8] = 0
    assert np.array_equal(host(pred, o, weight, quats, nq=nx), plant_residuals_host(pred, obs, w0, quats, nq=nx))

    # a whole quaternion: its four terms are +0.0, no flip is taken, and the other quaternion is aligned as before
    o = obs.copy()
    o[..., 4:8] = np.nan
    w0 = weight.copy()
    w0[4:8] = 0
    assert np.array_equal(host(pred, o, weight, quats, nq=nx), plant_residuals_host(pred, obs, w0, (0,), nq=nx))

    # a whole window: exactly +0.0 for every plant, sensors included
    o, s = obs.copy(), os_.copy()
    o[2], s[2] = np.nan, np.nan
    got = host(pred, o, weight, quats, nq=nx, pred_sens=ps, obs_sens=s, weight_sens=ws)
    assert np.array_equal(got[:, 2], np.zeros(M, dtype=np.float32)) and not np.signbit(got[:, 2]).any() and (np.delete(got, 2, axis=1) > 0).all()

    # a NaN prediction under an unreported entry stays finite (and changes nothing); under a reported one it gives NaN, in that (plant, window) alone
    o = obs.copy()
    o[3, 1, 8] = np.nan
    clean = host(pred, o, weight, quats, nq=nx, pred_sens=ps, obs_sens=os_, weight_sens=ws)
    bad = p4.copy()
    bad[1, 3, 1, 8] = np.nan
    assert np.array_equal(host(bad.reshape(M * W, H, nx), o, weight, quats, nq=nx, pred_sens=ps, obs_sens=os_, weight_sens=ws), clean) and np.isfinite(clean).all()
    bad[1, 3, 1, 7] = np.nan
    got = host(bad.reshape(M * W, H, nx), o, weight, quats, nq=nx, pred_sens=ps, obs_sens=os_, weight_sens=ws)
    assert np.isnan(got[1, 3]) and np.array_equal(np.delete(got.ravel(), 1 * W + 3), np.delete(clean.ravel(), 1 * W + 3))
    sb = ps.copy().reshape(M, W, H, ns)
    sb[2, 0, 0, 1] = np.nan
    s = os_.copy()
    s[0, 0, 1] = np.nan
    assert np.isnan(host(pred, o, weight, quats, nq=nx, pred_sens=sb.reshape(M * W, H, ns), obs_sens=os_, weight_sens=ws)[2, 0])
    assert np.isfinite(host(pred, o, weight, quats, nq=nx, pred_sens=sb.reshape(M * W, H, ns), obs_sens=s, weight_sens=ws)).all()


def test_restatement_refusals():
    from judo_amd.reports import plant_residuals_reports_host as host

    obs, w = np.zeros((2, 3, 8), np.float32), np.ones(8, np.float32)
    pred = np.zeros((4, 3, 8), np.float32)
    ps, os_, ws = np.zeros((4, 3, 2), np.float32), np.zeros((2, 3, 2), np.float32), np.ones(2, np.float32)
    assert host(pred, obs, w, (3,), nq=7, pred_sens=ps, obs_sens=os_, weight_sens=ws).shape == (2, 2)
    for kw, text in ((dict(pred=pred[:3]), "pred must be"), (dict(weight=w[:5]), "weight must have nx = 8"), (dict(nq=9), "nq = 9"), (dict(quat_adr=(4,), nq=7), r"quat_adr\[0\] = 4"),
                     (dict(quat_adr=(0, 3)), r"quat_adr\[1\] = 3 overlaps quat_adr\[0\] = 0"), (dict(obs=np.zeros((2, 65, 8), np.float32)), "JH_MAX_ID_HORIZON"),
                     (dict(pred_sens=ps), "all three or none"), (dict(pred_sens=ps[:3], obs_sens=os_, weight_sens=ws), "sensors:"),
                     (dict(pred_sens=ps, obs_sens=os_[:, :2], weight_sens=ws), "sensors:")):
        args = {**dict(pred=pred, obs=obs, weight=w, quat_adr=(), nq=None), **kw}
        with pytest.raises(ValueError, match=text):
            host(**args)


# ---- ReportEstimator ---------------------------------------------------------------------------------------------------------------------------------------------
def _host_set(task="cartpole", M=3, ns=None):
    """What a ReportEstimator reads of a GpuModelSet, on the CPU device."""
    import torch

    from judo_amd.models import layout, load_description

    desc = load_description(task)
    lay = layout(desc)
    model = SimpleNamespace(desc=desc, nq=lay.nq, nx=lay.nq + lay.nv, nu=lay.nu, ns=lay.ns if ns is None else ns, device=torch.device("cpu"))
    return SimpleNamespace(models=[model] * M)


def _estimator(errors=None, task="cartpole", M=3, ns=None, **kw):
    from judo_amd.reports import ReportEstimator

    est = ReportEstimator(_host_set(task, M, ns), **kw)
    if errors is not None:
        est._score = lambda: np.asarray(errors, dtype=np.float32)[:, -len(est):]
    return est


def _window(est, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal(est.nx), rng.standard_normal((est.horizon, est.nu)), rng.standard_normal((est.horizon, est.nx))


def test_observe_records_reports_and_counts_them():
    est = _estimator(task="fr3_pick", M=2, horizon=4, windows=3, sensor_sigma=0.5)
    assert est.ns == 14 and est.quat_adr == [3] and est.weight_sens.dtype == np.float32 and np.array_equal(est.weight_sens, np.full(14, 4.0, dtype=np.float32))
    assert est.reported.shape == (0,) and est.recorded_sensors().shape == (0, 4, 14)
    rng = np.random.default_rng(0)
    wins = []
    for i in range(5):
        x0, u, s = _window(est, i)
        y = rng.standard_normal((4, est.ns))
        s[1::2] = np.nan  # every second step
        s[:, est.nq :] = np.nan  # no velocities
        if i % 2:
            s[0, 3:7] = np.nan  # a whole quaternion
            y[:, ::2] = np.nan
        wins.append((x0, u, s, y if i != 3 else None))
        est.observe(x0, u, s, None if i == 3 else y)
        kept = wins[max(0, i - 2) : i + 1]
        _, _, states = est.recorded()
        assert np.array_equal(states, np.stack([k[2] for k in kept]).astype(np.float32), equal_nan=True)
        sens = np.stack([k[3] if k[3] is not None else np.full((4, est.ns), np.nan) for k in kept]).astype(np.float32)
        assert np.array_equal(est.recorded_sensors(), sens, equal_nan=True)
        want = [int((~np.isnan(k[2])).sum() + (0 if k[3] is None else (~np.isnan(k[3])).sum())) for k in kept]
        assert est.reported.tolist() == want and est.reported.dtype == np.int64
    assert est.reported.tolist()[1] == 2 * est.nq - 4  # (window 3: two reported rows of positions, one without its quaternion, no sensors)
    est = _estimator(horizon=2, windows=2)  # sensors no evidence: nothing recorded for them
    x0, u, s = _window(est, 0)
    s[:] = np.nan
    est.observe(x0, u, s)
    assert est.reported.tolist() == [0] and est.recorded_sensors() is None and est._obs_sens is None


def test_start_and_step_record_the_windows_observe_would():
    est, ref = _estimator(horizon=3, windows=4), _estimator(horizon=3, windows=4)
    assert est.needs_start and est.window_steps == 0
    with pytest.raises(ValueError, match="no window is pending.*start"):
        est.step(np.zeros(est.nu))
    rng = np.random.default_rng(1)
    xs, us = rng.standard_normal((10, est.nx)), rng.standard_normal((10, est.nu))
    est.start(xs[0])
    assert not est.needs_start
    est.step(us[0])  # no report
    partial = xs[2].copy()
    partial[est.nq :] = np.nan
    est.step(us[1], partial)  # positions only
    assert est.window_steps == 2 and len(est) == 0
    est.step(us[2], xs[3])  # a full state ends the window: it starts the next
    assert len(est) == 1 and not est.needs_start and est.window_steps == 0
    ref.observe(xs[0], us[:3], np.stack([np.full(est.nx, np.nan), partial, xs[3]]))
    for t in (3, 4):
        est.step(us[t], xs[t + 1])
    est.step(us[5], partial)  # the window ends in a partial report: the next state is unknown
    assert len(est) == 2 and est.needs_start
    ref.observe(xs[3], us[3:6], np.stack([xs[4], xs[5], partial]))
    with pytest.raises(ValueError, match="no window is pending"):
        est.step(us[6], xs[7])
    est.start(xs[6])
    est.step(us[6], xs[7])
    est.start(xs[7])  # a pending window is dropped
    assert est.window_steps == 0 and len(est) == 2
    for t in (7, 8, 9):
        est.step(us[t])
    assert len(est) == 3 and est.needs_start  # a window with nothing reported is recorded: no evidence
    ref.observe(xs[7], us[7:10], np.full((3, est.nx), np.nan))
    for a, b in zip(est.recorded(), ref.recorded()):
        assert np.array_equal(a, b, equal_nan=True)
    assert est.reported.tolist() == ref.reported.tolist() == [est.nx + est.nq, 2 * est.nx + est.nq, 0]
    # the inherited full-state observe_step keeps working, and its windows count as fully reported
    est.observe_step(xs[0], us[0], xs[1])
    est.observe_step(xs[1], us[1], xs[2])
    est.observe_step(xs[2], us[2], xs[3])
    assert len(est) == 4 and est.reported.tolist()[-1] == 3 * est.nx
    est.reset()
    assert len(est) == 0 and est.needs_start and est.reported.shape == (0,)

    est = _estimator(task="fr3_pick", M=2, horizon=2, windows=2, sensor_sigma=1.0)  # sensors through step
    x = np.random.default_rng(2).standard_normal(est.nx)
    y = np.arange(est.ns, dtype=np.float64)
    est.start(x)
    est.step(np.zeros(est.nu), None, y)
    est.step(np.zeros(est.nu), x)
    assert len(est) == 1 and est.reported.tolist() == [est.ns + est.nx]
    assert np.array_equal(est.recorded_sensors()[0], np.stack([y, np.full(est.ns, np.nan)]).astype(np.float32), equal_nan=True)


def test_report_estimator_refusals():
    for kw, text in ((dict(ns=0, sensor_sigma=1.0), "sensor_sigma = 1.0 for a model without sensors"), (dict(task="fr3_pick", sensor_sigma=0.0), "sensor_sigma must be a positive"),
                     (dict(task="fr3_pick", sensor_sigma=[1.0, 2.0]), r"sensor_sigma must be a positive, finite scalar or \(14,\) vector"),
                     (dict(task="fr3_pick", sensor_sigma=np.nan), "sensor_sigma"), (dict(state_sigma=0.0), "state_sigma"), (dict(horizon=65), "horizon = 65.*JH_MAX_ID_HORIZON"),
                     (dict(windows=0), "windows = 0"), (dict(prior=[0.5, 0.5]), "prior has 2 entries for M = 3")):
        with pytest.raises(ValueError, match=text):
            _estimator(**kw)
    est = _estimator(task="fr3_pick", M=2, horizon=4, windows=2)
    x0, u, s = _window(est, 0)

    def bad(a, idx):
        a = a.copy()
        a[idx] = np.nan
        return a

    part = s.copy()
    part[2, 4] = np.nan  # one coordinate of the free joint's quaternion
    for args, text in (((bad(x0, 5), u, s), "x0 holds NaN"), ((x0, bad(u, (1, 0)), s), "controls hold NaN"),
                       ((x0, u, part), "quaternion at offset 3 is reported in part in row 2 .1 of its four"), ((x0, u, s, np.zeros((4, est.ns))), "sensor_sigma = None"),
                       ((x0[:3], u, s), "x0 must be"), ((x0, u[:3], s), r"controls must be \(horizon, nu\)"), ((x0, u, s[:3]), r"states must be \(horizon, nx\)")):
        with pytest.raises(ValueError, match=text):
            est.observe(*args)
    assert len(est) == 0
    with pytest.raises(ValueError, match="x holds NaN"):
        est.start(bad(x0, 0))
    with pytest.raises(ValueError, match="x must be"):
        est.start(x0[:4])
    est.start(x0)
    for args, text in (((bad(u[0], 0),), "u holds NaN"), ((u[0, :2],), "u must be"), ((u[0], s[0, :5]), "report must be"), ((u[0], part[2]), "reported in part"),
                       ((u[0], None, np.zeros(est.ns)), "sensor_sigma = None")):
        with pytest.raises(ValueError, match=text):
            est.step(*args)
    assert est.window_steps == 0
    est = _estimator(task="fr3_pick", M=2, horizon=4, windows=2, sensor_sigma=1.0)
    with pytest.raises(ValueError, match=r"sensors must be \(horizon, ns\) = \(4, 14\)"):
        est.observe(x0, u, s, np.zeros((4, 3)))
    est.start(x0)
    with pytest.raises(ValueError, match=r"sensors must be \(ns,\) = \(14,\)"):
        est.step(u[0], None, np.zeros(3))


def _assignment_controller(M=3, blocks=8):
    from judo_amd.plants import Assignment

    class Ctrl(Assignment):
        def __init__(self):
            self._descriptions = [{}] * M
            self._init_assignment(blocks, None, M)

    return Ctrl()


def _risk_controller(M=3):
    from judo_amd.plants import WorstCase

    class Ctrl(WorstCase):
        def __init__(self):
            self.calls = []

        def set_weights(self, w, tail=None):
            self.calls.append((np.array(w), tail))

    return Ctrl()


def _hand_over(est):
    ctrl = _assignment_controller()
    w = est.apply(ctrl, floor=0.25)
    assert np.array_equal(est.posterior, [0.0, 0.0, 1.0])
    np.testing.assert_allclose(w, [1 / 12, 1 / 12, 10 / 12], rtol=1e-15)
    assert ctrl.assignment == [0, 1, 2, 2, 2, 2, 2, 2]
    risk = _risk_controller()
    w = est.apply_risk(risk, floor=0.1, tail=0.5)
    np.testing.assert_allclose(w, [0.1 / 3, 0.1 / 3, 0.9 + 0.1 / 3], rtol=1e-15)
    assert len(risk.calls) == 1 and np.array_equal(risk.calls[0][0], w) and risk.calls[0][1] == 0.5
    with pytest.raises(ValueError, match="an ensemble controller"):
        est.apply(risk)
    with pytest.raises(ValueError, match="no risk measure over its plants.*follows the belief with apply"):
        est.apply_risk(ctrl)


def test_apply_and_apply_risk_on_stand_ins():
    est = _estimator([[np.inf], [np.inf], [0.0]], horizon=2, windows=4)
    x0, u, s = _window(est, 0)
    s[0] = np.nan
    est.observe(x0, u, s)
    _hand_over(est)
    assert est.map == 2 and est.errors.shape == (3, 1)


# ---- SpotReportEstimator -----------------------------------------------------------------------------------------------------------------------------------------
def _spot_stub(task="spot_box", M=3, ns=None):
    """What a SpotReportEstimator reads of a SpotPlantSet before its first launch, on the CPU device."""
    import torch

    from judo_amd.models import layout, load_description

    desc = load_description(task)
    lay = layout(desc)
    return SimpleNamespace(descriptions=[desc] * M, num_plants=M, nq=lay.nq, nv=lay.nv, nsensordata=lay.ns if ns is None else ns, device=torch.device("cpu"))


def test_spot_windows_and_quaternion_offsets_on_a_stub_set():
    from judo_amd.reports import SpotReportEstimator

    stub = _spot_stub()
    est = SpotReportEstimator(stub, horizon=2, windows=3)
    assert (est.nq, est.nv, est.nx, est.num_plants) == (33, 31, 64, 3) and est.quat_adr == [3, 29] and est.physics_substeps == 2 and est.horizon == 2
    assert SpotReportEstimator(_spot_stub("spot", 2)).quat_adr == [3] and SpotReportEstimator(_spot_stub("spot", 2)).horizon == 4
    assert est.update().tolist() == [1 / 3] * 3 and est.recorded()[3].shape == (0, 2, 64) and est.recorded()[4] is None
    rng = np.random.default_rng(0)
    wins = []
    for i in range(4):
        w = [rng.standard_normal(64), rng.standard_normal((2, 25)), rng.standard_normal(12), rng.standard_normal((2, 64))]
        w[3][:, 33:] = np.nan  # no velocities
        if i == 1:
            w[3][:, :26] = np.nan  # the object's pose is the only report
        if i == 2:
            w[3][0, 3:7] = np.nan  # the base's orientation dropped in one row
        wins.append(w)
        est.observe(*w)
        kept = wins[max(0, i - 2) : i + 1]
        for got, k in zip(est.recorded()[:4], zip(*kept)):
            assert got.dtype == np.float32 and np.array_equal(got, np.stack(k).astype(np.float32), equal_nan=True)
        assert est.reported.tolist() == [int((~np.isnan(k[3])).sum()) for k in kept]
    assert est.reported.tolist() == [14, 62, 66] and len(est) == 3
    assert est.chunks(90) == [(0, 85), (85, 90)] and est.chunks(16) == [(0, 16)] and est.chunks() == [(0, 3)]
    est._score = lambda: np.asarray([[np.inf] * 3, [np.inf] * 3, [0.0] * 3], dtype=np.float32)
    _hand_over(est)

    est = SpotReportEstimator(_spot_stub(ns=5), horizon=2, windows=2, sensor_sigma=[1, 1, 2, 2, 4], state_sigma=0.5)
    assert np.array_equal(est.weight_sens, np.array([1, 1, 0.25, 0.25, 0.0625], dtype=np.float32)) and np.array_equal(est.weight, np.full(64, 4.0, dtype=np.float32))
    w = wins[0]
    est.observe(*w)
    y = rng.standard_normal((2, 5))
    y[1, 2] = np.nan
    est.observe(*w, y)
    sens = est.recorded()[4]
    assert np.isnan(sens[0]).all() and np.array_equal(sens[1], y.astype(np.float32), equal_nan=True) and est.reported.tolist() == [66, 66 + 9]


def test_spot_refusals():
    from judo_amd.reports import SpotReportEstimator

    stub = _spot_stub()
    for kw, text in ((dict(horizon=65), "horizon = 65.*JH_MAX_ID_HORIZON"), (dict(horizon=0), "horizon = 0"), (dict(windows=0), "windows = 0"),
                     (dict(physics_substeps=0), "physics_substeps = 0"), (dict(state_sigma=-1.0), "state_sigma"), (dict(sensor_sigma=0.0), "sensor_sigma"),
                     (dict(prior=[1, 1]), "prior has 2 entries for M = 3"), (dict(temperature=0.0), "temperature = 0.0"), (dict(discount=2.0), "discount = 2.0")):
        with pytest.raises(ValueError, match=text):
            SpotReportEstimator(_spot_stub(ns=5), **kw)
    with pytest.raises(ValueError, match="sensor_sigma = 1.0 for a model without sensors"):
        SpotReportEstimator(_spot_stub(ns=0), sensor_sigma=1.0)
    with pytest.raises(ValueError, match="plants must be a SpotPlantSet, got list"):
        SpotReportEstimator([1, 2])
    with pytest.raises(ValueError, match="M = 33 exceeds"):
        SpotReportEstimator(_spot_stub(M=33))
    with pytest.raises(ValueError, match="ctrl is a SimpleNamespace, which plans on no SpotPlantSet"):
        SpotReportEstimator.for_controller(SimpleNamespace(model_set=None))
    est = SpotReportEstimator(stub, horizon=2, windows=2)
    rng = np.random.default_rng(1)
    x0, cmd, out, s = rng.standard_normal(64), rng.standard_normal((2, 25)), rng.standard_normal(12), rng.standard_normal((2, 64))

    def bad(a, idx):
        a = a.copy()
        a[idx] = np.nan
        return a

    for args, text in (((bad(x0, 0), cmd, out, s), "x0 holds NaN"), ((x0, bad(cmd, (0, 0)), out, s), "commands holds NaN"), ((x0, cmd, bad(out, 3), s), "last_policy_output holds NaN"),
                       ((x0, cmd, out, bad(s, (1, 30))), "quaternion at offset 29 is reported in part in row 1"), ((x0, cmd, out, bad(s, (0, 3))), "quaternion at offset 3"),
                       ((x0, cmd, out, s, np.zeros((2, 5))), "sensor_sigma = None"), ((x0[:5], cmd, out, s), "x0 must be"), ((x0, cmd[:, :24], out, s), r"commands must be \(horizon, 25\)"),
                       ((x0, cmd, out[:3], s), "last_policy_output must be"), ((x0, cmd, out, s[:1]), "states must be")):
        with pytest.raises(ValueError, match=text):
            est.observe(*args)
    assert len(est) == 0
