"""judo_amd.reports.SpotReportEstimator on the device: W recorded windows of T control steps rolled out on the M plants of a SpotPlantSet in one
jh_policy_rollout_plants chain (a problem per window, a block per plant) and scored by jh_plant_residuals_reports with window-major strides.

The observed states of a case are jh_policy_rollout with N = 1 on the true plant's OWN engine, from a zero warm start at every control step and with the set's
self-collision switch -- the reference, not the code under test.  The chain on the set is bit for bit that rollout (tests/test_gpu_tree_plants.py), so the true plant's
error is exactly 0.0 and needs no tolerance; the other plants' errors are the numpy restatement's on the single-engine rollouts, bit for bit.

spot_box (nq / nv = 33 / 31), M = 3 plants scaled in box mass, box friction and actuator_kp, W = 2 windows of T = 2 control steps of 2 substeps, the box where the robot
touches it.  No deadline: timing cannot enter the results."""

import functools
from types import SimpleNamespace

import numpy as np
import pytest

from tests import test_gpu_spot_plant_controllers as ctl
from tests import test_gpu_tree_plants as tree

pytestmark = pytest.mark.gpu

M, W, T, SUBSTEPS = 3, 2, 2, 2
NQ, NV = 33, 31
# The truth is noise-free and the plants part slowly: after T * SUBSTEPS = 4 physics steps the box's pose differs between two plants by far less than the robot's joints
# do.  At sigma = 1 a wrong plant's L = 0.5 * sum of squares falls below 2**-53 and exp(-L) is 1.0 in fp64: a tie, not a MAP.  sigma = 1e-4, the order of an encoder's
# resolution, weighs the squares by 1e8.
SIGMA = 1e-4
WEIGHT = np.float32(1) / (np.full(NQ + NV, SIGMA).astype(np.float32) * np.full(NQ + NV, SIGMA).astype(np.float32))  # 1 / sigma**2, in fp32


@functools.lru_cache(maxsize=None)
def _plants(self_collision=True):
    """The set of M = 3 spot_box plants: the task's description, tests/test_gpu_tree_plants.py's scaling, and that scaling halved."""
    from judo_amd.models import scaled_description
    from judo_amd.policy import SpotPlantSet

    base, full = tree._task("spot_box").desc, tree.KINDS["spot_box"][1]
    half = {k: {name: 1.0 + (f - 1.0) / 2 for name, f in v.items()} for k, v in full.items()}
    return SpotPlantSet([base, scaled_description(base, **full), scaled_description(base, **half)], self_collision=self_collision)


def _single(engine, x0, commands, policy_out):
    """jh_policy_rollout with N = 1 on `engine`, window by window: (W, T, nx) states and (W, T, ns) sensors as fp32 host arrays."""
    import torch

    from judo_amd.policy import PolicyRolloutBackend

    pb = PolicyRolloutBackend(1, physics_substeps=SUBSTEPS, carry_warmstart=False, share=SimpleNamespace(device=engine.device, engine=engine, policy=tree._policy()))
    states, sensors = [], []
    for w in range(x0.shape[0]):
        s, y, _ = pb.rollout(x0[w], commands[w : w + 1], policy_out[w : w + 1])
        states.append(s[0])
        sensors.append(y[0])
    torch.cuda.synchronize()
    return torch.stack(states).cpu().numpy(), torch.stack(sensors).cpu().numpy()


def _windows(rows, steps, seed):
    """(x0 (rows, nx), commands (rows, steps, 25), last policy outputs (rows, 12)) on the device: tests/test_gpu_tree_plants.py's start states and commands."""
    import torch

    x0, commands = tree._states("spot_box", rows, seed), tree._commands(rows, seed + 1)[:, :steps].contiguous()
    out = 0.1 * np.random.default_rng(seed + 2).standard_normal((rows, 12))
    return x0, commands, torch.as_tensor(out, dtype=torch.float32, device="cuda")


@functools.lru_cache(maxsize=None)
def _reference():
    """The case, computed once and left unchanged: the windows and every plant's own single-engine rollout of them.  Every two plants roll out differently."""
    ps = _plants()
    assert (ps.nq, ps.nv, ps.num_plants) == (NQ, NV, M)
    x0, commands, out = _windows(W, T, 11)
    obs, sens = zip(*[_single(ps.engines[m], x0, commands, out) for m in range(M)])
    for a in range(M):
        assert np.isfinite(obs[a]).all() and np.isfinite(sens[a]).all()
    return dict(ps=ps, x0=x0.cpu().numpy(), commands=commands.cpu().numpy(), out=out.cpu().numpy(), obs=obs, sens=sens)


def _thin(obs, what):
    o = obs.copy()
    if what in ("positions", "object"):
        o[..., NQ:] = np.nan  # no velocities
    if what == "object":
        o[..., :26] = np.nan  # the robot's own joints and base unreported: the box's pose from perception is the only report
    return o


def _estimator(ref, observed, sensors=None, plants=None, windows=None, **kw):
    from judo_amd.reports import SpotReportEstimator

    n = len(observed)
    est = SpotReportEstimator(plants or ref["ps"], horizon=observed.shape[1], windows=windows or n, physics_substeps=SUBSTEPS, policy=tree._policy(), state_sigma=SIGMA, **kw)
    assert est.weight.tobytes() == WEIGHT.tobytes()
    for w in range(n):
        est.observe(ref["x0"][w], ref["commands"][w], ref["out"][w], observed[w], None if sensors is None else sensors[w])
    assert len(est) == min(n, est.windows)
    return est


def _window_major(per_plant):
    """M arrays (W, T, n) -> (W * M, T, n), row w * M + m."""
    return np.ascontiguousarray(np.stack(per_plant, axis=1)).reshape((-1,) + per_plant[0].shape[1:])


@pytest.mark.parametrize("what", ["full", "positions", "object"])
def test_the_true_plant_has_error_zero_and_is_the_map(gpu, what):
    from judo_amd.reports import plant_residuals_reports_host

    ref = _reference()
    thin = [_thin(ref["obs"][j], what) for j in range(M)]
    for a in range(M):  # the condition of the test: every two plants differ in the reported entries
        for b in range(a + 1, M):
            assert not np.array_equal(thin[a], thin[b], equal_nan=True), f"plants {a} and {b} report alike ({what}): the case shows nothing"
    for j in range(M):
        est = _estimator(ref, thin[j])
        assert est.quat_adr == [3, 29] and est.reported.tolist() == [T * {"full": NQ + NV, "positions": NQ, "object": 7}[what]] * W
        post = est.update()
        print(f"{what}: true plant {j}: errors per plant {est.errors.sum(axis=1)}, posterior {post}")
        assert est.errors.shape == (M, W) and est.errors.dtype == np.float32
        assert np.array_equal(est.errors[j], np.zeros(W, dtype=np.float32)), f"{what}: true plant {j}: errors {est.errors[j]}"
        for m in range(M):
            assert m == j or est.errors[m].sum() > 0, f"{what}: plant {m} is told from true plant {j} by nothing"
        assert est.map == j and post.argmax() == j and not est.degenerate and abs(post.sum() - 1) < 1e-12
        want = plant_residuals_reports_host(_window_major(ref["obs"]), thin[j], WEIGHT, est.quat_adr, nq=NQ, window_major=True)
        np.testing.assert_array_equal(est.errors.view(np.uint32), want.view(np.uint32), err_msg=f"{what}: true plant {j}")


def test_sensors_are_evidence(gpu):
    """No state reported at all, the sensor readings of every second control step: bits against the restatement, the truth the MAP."""
    from judo_amd.reports import plant_residuals_reports_host

    ref = _reference()
    ns = ref["sens"][0].shape[-1]
    nothing = np.full((W, T, NQ + NV), np.nan, dtype=np.float32)
    y = ref["sens"][1].copy()
    y[:, 0] = np.nan
    assert not np.array_equal(ref["sens"][0][:, 1], y[:, 1]) and not np.array_equal(ref["sens"][2][:, 1], y[:, 1])
    est = _estimator(ref, nothing, y, sensor_sigma=0.5)
    est.update()
    want = plant_residuals_reports_host(_window_major(ref["obs"]), nothing, WEIGHT, est.quat_adr, nq=NQ, pred_sens=_window_major(ref["sens"]),
                                        obs_sens=y, weight_sens=np.full(ns, 4.0, dtype=np.float32), window_major=True)
    np.testing.assert_array_equal(est.errors.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(est.errors[1], np.zeros(W, dtype=np.float32)) and est.map == 1 and est.errors[0].sum() > 0 and est.errors[2].sum() > 0
    assert est.reported.tolist() == [ns] * W


def test_more_pairs_than_one_chain_holds(gpu, monkeypatch):
    """W = 90 windows of T = 1 at M = 3 are 270 (window, plant) blocks, above JH_MAX_FLEET_PLANT_BLOCKS = 256: the first chain holds 85 windows, the second 5.  The
    result is the unchunked restatement's on the single-engine rollouts."""
    from judo_amd import _lib
    from judo_amd.reports import plant_residuals_reports_host

    ps, n = _plants(), 90
    x0, commands, out = _windows(n, 1, 21)
    obs = [_single(ps.engines[m], x0, commands, out)[0] for m in range(M)]
    ref = dict(ps=ps, x0=x0.cpu().numpy(), commands=commands.cpu().numpy(), out=out.cpu().numpy())
    thin = _thin(obs[2], "positions")
    est = _estimator(ref, thin)
    assert n * M > _lib.MAX_FLEET_PLANT_BLOCKS and est.chunks() == [(0, 85), (85, 90)]
    L = _lib.lib()
    calls, plants = [], L.jh_policy_rollout_plants

    def count(*a):
        calls.append((a[2], a[3]))  # (B, G)
        return plants(*a)

    monkeypatch.setattr(L, "jh_policy_rollout_plants", count)
    est.update()
    monkeypatch.undo()
    assert calls == [(85, M), (5, M)]
    want = plant_residuals_reports_host(_window_major(obs), thin, WEIGHT, est.quat_adr, nq=NQ, window_major=True)
    np.testing.assert_array_equal(est.errors.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(est.errors[2], np.zeros(n, dtype=np.float32)) and est.map == 2 and (est.errors[:2].sum(axis=1) > 0).all()


def _carried(c):
    """Everything a Spot plant controller carries from one plan step to the next, as bytes."""
    parts = [c._last_policy_output, c.rollout_backend._warm]
    if getattr(c, "_plant_backend", None) is not None:
        parts += [c._plant_policy_out, c._plant_backend._warm]
    return [p.cpu().numpy().tobytes() for p in parts]


def _record(est, ctrl, truth, rows=2):
    """`rows` windows of T control steps as plant `truth` of the controller's set answers them, positions only."""
    import torch

    x0 = torch.as_tensor(np.stack([ctl._state(ctrl.task, 20 + w) for w in range(rows)]), dtype=torch.float32, device="cuda")
    _, commands, out = _windows(rows, T, 31)
    obs, _ = _single(ctrl.plants.engines[truth], x0, commands, out)
    for w in range(rows):
        est.observe(x0[w], commands[w], out[w], _thin(obs[w], "positions"))


@pytest.mark.parametrize("kind", ["ensemble", "randomized"])
def test_for_controller(gpu, kind):
    """The smallest sizes of tests/test_gpu_spot_plant_controllers.py.  The estimator follows `set_member`, hands its posterior over, and leaves what the controller
    carries alone: a twin that never saw an estimator plans the same bits over two plan steps as one with an `update()` between them."""
    from judo_amd.reports import SpotReportEstimator

    descs = ctl._descs("spot_box_push", M)
    make = (lambda: ctl._ensemble("spot_box_push", "mppi", descs)) if kind == "ensemble" else (lambda: ctl._randomized("spot_box_push", "mppi", descs, blocks=M))
    ctrl, twin = make(), make()
    est = SpotReportEstimator.for_controller(ctrl, horizon=T, windows=4, state_sigma=1e-5)
    assert est.physics_substeps == ctrl.rollout_backend.physics_substeps and est._policy is ctrl.rollout_backend.policy and est.plants is ctrl.plants
    _record(est, ctrl, truth=2)
    for c in (ctrl, twin):
        c.update_action()
    before = _carried(ctrl)
    est.update()
    print(f"{kind}: errors per plant {est.errors.sum(axis=1)}, posterior {est.posterior}")
    assert np.array_equal(est.errors[2], np.zeros(2, dtype=np.float32)) and est.map == 2 and (est.errors[:2].sum(axis=1) > 0).all()
    assert _carried(ctrl) == before == _carried(twin)
    for c in (ctrl, twin):
        ctl._set_state(c, 1)
        c.update_action()
    ctl._assert_same(ctl._snapshot(ctrl), ctl._snapshot(twin), f"{kind}: a twin without an estimator")
    assert _carried(ctrl) == _carried(twin)

    if kind == "ensemble":
        w = est.apply_risk(ctrl, floor=0.1)
        np.testing.assert_allclose(ctrl.weights, w / w.sum(), rtol=2.0**-23)  # (normalised in fp64, rounded to fp32)
        assert w.argmax() == 2
        with pytest.raises(ValueError, match="an ensemble controller"):
            est.apply(ctrl)
    else:
        w = est.apply(ctrl, floor=0.25)
        np.testing.assert_allclose(w, [1 / 12, 1 / 12, 10 / 12], atol=0.01)
        assert ctrl.assignment == [2, 2, 2]
        with pytest.raises(ValueError, match="no risk measure over its plants"):
            est.apply_risk(ctrl)
    ctrl.set_member(1, descs[2])  # plant 1 is now the truth as well
    post = est.update()
    assert np.array_equal(est.errors[1], est.errors[2]) and np.array_equal(est.errors[1], np.zeros(2, dtype=np.float32)) and post[1] == post[2] and est.errors[0].sum() > 0
    ctrl.update_action()
    assert np.isfinite(ctrl.nominal_knots).all()
