"""judo_amd.simulation on the device: `GpuSimulation.step` against `GpuRolloutBackend.rollout`, and `ClosedLoop` against loops written out by hand -- a plain
`Controller` per plant and jh_rollout_materialize on the plant's own handle (tests/test_gpu_materialize_plants.py `_single`), which are the parent's entries alone."""

import numpy as np
import pytest

from tests import test_gpu_materialize_plants as closed

pytestmark = pytest.mark.gpu

N, H, S, PERIODS = 32, 8, 4, 3
TRUTH = [2, 0, 1]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize("name", ["cartpole", "leap_cube"])
def test_step_equals_the_rollout_backend(gpu, name):
    """Two chained steps from a state of the task (leap_cube: the cube resting on the fingers): each equals `GpuRolloutBackend.rollout` at N = 1, H = 1."""
    from judo_amd.rollout_backend import GpuRolloutBackend
    from judo_amd.simulation import GpuSimulation

    sim = GpuSimulation(name)
    x = closed._x0(name, 1, 7)[0].astype(np.float64)
    us = closed._controls(name, 1, 2, 8)[0].astype(np.float64)
    sim.task.data.qpos, sim.task.data.qvel, sim.task.data.time = x[: sim.task.nq].copy(), x[sim.task.nq :].copy(), 0.0
    backend = GpuRolloutBackend(name, 1)
    for t in range(2):
        sim.step(us[t])
        want = backend.rollout(x, us[t][None, None])[0][0, 0]
        got = np.concatenate([sim.sim_state.qpos, sim.sim_state.qvel])
        assert np.isfinite(want).all() and not np.array_equal(want, x)
        np.testing.assert_array_equal(got, want, err_msg=f"{name} step {t}")
        assert sim.sim_state.time == pytest.approx((t + 1) * sim.timestep, abs=1e-12)
        x = want
    sim.pause()
    sim.step(us[0])
    assert np.array_equal(np.concatenate([sim.sim_state.qpos, sim.sim_state.qvel]), x)


def test_a_description_makes_another_plant(gpu):
    from judo_amd.simulation import GpuSimulation
    from tests.test_gpu_plant_estimator import _cartpole_descriptions, _reference

    import torch

    descs, models = _cartpole_descriptions(), _reference("cartpole")["models"]
    x = closed._x0("cartpole", 1, 9)[0]
    u = closed._controls("cartpole", 1, 1, 10)
    out = []
    for desc in (None, descs[2]):
        sim = GpuSimulation("cartpole", description=desc)
        sim.task.data.qpos, sim.task.data.qvel = x[:2].astype(np.float64), x[2:].astype(np.float64)
        sim.step(u[0, 0])
        out.append(np.concatenate([sim.sim_state.qpos, sim.sim_state.qvel]).astype(np.float32))
    assert not np.array_equal(out[0], out[1])
    for got, model in zip(out, (models[0], models[2])):
        want = closed._single(model, torch.from_numpy(x).to(gpu), 0, torch.from_numpy(u).to(gpu), want_sensors=False)[0][0, 0].cpu().numpy()
        np.testing.assert_array_equal(_bits(got), _bits(want))


def _configure(c, i):
    c.optimizer.config.num_rollouts = N
    c.controller_cfg.horizon = H * c.task.dt
    c.controller_cfg.max_opt_iters = 1
    np.random.seed(100 + i)  # (Task.reset draws the start state from numpy's global stream)
    c.reset()
    c.optimizer.seed(1000 + 17 * i)


def _lone_loop(ref, c, plant, x, delay):
    """One controller against one plant, written out: update_states, update_action, the spline at the plant's clock through the restatement, the plant's own
    jh_rollout_materialize launch for the segment, Task.reward.  Returns (states (PERIODS * S, nx), the return)."""
    import torch

    from judo_amd.simulation import plant_controls_host, spline_rows

    model, dt, nq = ref["models"][plant], ref["models"][plant].dt, ref["models"][plant].nq
    total, count, traj = 0.0, 0, []
    for _ in range(PERIODS):
        t = 0.0 + count * dt
        c.update_states(x[:nq].astype(np.float64), x[nq:].astype(np.float64), float(t), {})
        old = c.spline_data
        c.update_action()
        rows = [plant_controls_host(*spline_rows([old], [t], dt, 0, delay))] if delay else []
        controls = np.concatenate(rows + [plant_controls_host(*spline_rows([c.spline_data], [t], dt, delay, S))], axis=1)
        u_d = torch.from_numpy(controls).to(model.device)
        states, sensors = closed._single(model, torch.from_numpy(np.ascontiguousarray(x)).to(model.device), 0, u_d)
        total += float(c.task.reward(states, sensors, u_d, {}).cpu().numpy()[0])
        x = states[0, -1].cpu().numpy()
        traj.append(states[0].cpu().numpy())
        count += S
    return np.concatenate(traj), total


@pytest.mark.parametrize("delay", [0, 2])
def test_closed_loop_of_a_fleet_equals_three_lone_loops(gpu, delay):
    """Three cartpole controllers in a `ControllerFleet` on plants [2, 0, 1] of the estimator tests' set, three periods of S = 4: every nominal, every state and every
    return bit for bit where the three loops written out by hand leave them; likewise with a plan that takes effect two steps late."""
    from judo_amd.controller import make_controller
    from judo_amd.fleet import make_controller_fleet
    from judo_amd.simulation import ClosedLoop, PlantFleet
    from tests.test_gpu_plant_estimator import _reference

    ref = _reference("cartpole")
    x0 = closed._x0("cartpole", 3, 21)
    fleet = make_controller_fleet("cartpole", "mppi", 3)
    alone = [make_controller("cartpole", "mppi") for _ in range(3)]
    for i in range(3):
        _configure(fleet[i], i)
        _configure(alone[i], i)
    loop = ClosedLoop(fleet, PlantFleet(ref["mset"], TRUTH, x0), steps_per_plan=S, plan_delay=delay)
    assert ClosedLoop(fleet, loop.plants).steps_per_plan == 1  # round(1 / (20 Hz * 0.04 s)) = 1 for cartpole
    returns = loop.run(PERIODS)
    states, controls = loop.trajectory()
    assert states.shape == (3, PERIODS * S, 4) and controls.shape == (3, PERIODS * S, 1) and len(loop.plan_ms) == PERIODS and np.isfinite(returns).all()
    for b in range(3):
        want_states, want_return = _lone_loop(ref, alone[b], TRUTH[b], x0[b], delay)
        np.testing.assert_array_equal(_bits(states[b]), _bits(want_states), err_msg=f"plant {b}: states")
        assert fleet[b].nominal_knots.tobytes() == alone[b].nominal_knots.tobytes() and np.array_equal(fleet[b].times, alone[b].times), f"plant {b}: nominal"
        assert returns[b] == want_return, (b, returns[b], want_return)
    assert len({states[b].tobytes() for b in range(3)}) == 3
    np.testing.assert_array_equal(_bits(loop.plants.x_host()), _bits(states[:, -1]))


def _report_loop(ref, controllers, periods, after=None):
    """A loop on the estimator tests' plants that reports every second step without velocities, an estimator of that file's horizon, window count and sigma per plant."""
    from judo_amd.reports import ReportEstimator
    from judo_amd.simulation import ClosedLoop, PlantFleet
    from tests.test_gpu_plant_estimator import W

    plants = PlantFleet(ref["mset"], TRUTH, closed._x0("cartpole", 3, 31))
    plants.reports(every=2, columns=range(ref["models"][0].nq))
    members = controllers.controllers if hasattr(controllers, "controllers") else controllers
    ests = [ReportEstimator.for_controller(c, horizon=ref["H"], windows=W) if hasattr(c, "model_set") else ReportEstimator(ref["mset"], horizon=ref["H"], windows=W) for c in members]
    loop = ClosedLoop(controllers, plants, steps_per_plan=ref["H"], estimators=ests, after_period=after)
    loop.run(periods)
    return loop, ests


def test_report_estimators_in_the_loop_find_each_plants_truth(gpu):
    """Every second step, no velocities, W windows of the estimator tests' horizon: the plants launch of the estimator and the plants launch of the fleet are both bit
    for bit the plant's own launch, so the true plant's error is exactly 0.0 in every window and it is the MAP."""
    from judo_amd.controller import make_controller
    from tests.test_gpu_plant_estimator import M, W, _reference

    ref = _reference("cartpole")
    ctrls = [make_controller("cartpole", "mppi") for _ in range(3)]
    for i, c in enumerate(ctrls):
        _configure(c, i)
    loop, ests = _report_loop(ref, ctrls, W)
    nq, H = ref["models"][0].nq, ref["H"]
    for b, est in enumerate(ests):
        post = est.update()
        assert len(est) == W and est.reported.tolist() == [(H // 2) * nq] * W
        assert np.array_equal(est.errors[TRUTH[b]], np.zeros(W, dtype=np.float32)), (b, est.errors)
        assert all(m == TRUTH[b] or est.errors[m].sum() > 0 for m in range(M))
        assert est.map == TRUTH[b] and post.argmax() == TRUTH[b] and not est.degenerate


def test_a_weighted_ensemble_fleet_follows_its_estimators(gpu):
    """`apply_risk` inside the loop, after every period: each member of a `WeightedEnsembleFleet` plans the next period under its own posterior.  The results are finite
    and every member carries weights; nothing is claimed about who earns more."""
    from judo_amd.weighted_fleet import make_weighted_ensemble_fleet
    from tests.test_gpu_plant_estimator import W, _cartpole_descriptions, _reference

    ref = _reference("cartpole")
    fleet = make_weighted_ensemble_fleet("cartpole", "mppi", 3, _cartpole_descriptions(), worst=1)
    for i in range(3):
        _configure(fleet[i], i)
    holder = {}

    def follow(loop, period):
        for b, est in enumerate(loop.estimators):
            est.update()
            holder[b] = est.apply_risk(fleet[b], floor=0.1)

    loop, ests = _report_loop(ref, fleet, W, after=follow)
    assert np.isfinite(loop.returns).all() and np.isfinite(loop.trajectory()[0]).all()
    for b in range(3):
        assert np.isfinite(fleet[b].nominal_knots).all() and fleet[b].weights is not None and abs(float(fleet[b].weights.sum()) - 1) < 1e-6
        assert ests[b].map == TRUTH[b] and np.argmax(holder[b]) == TRUTH[b]
