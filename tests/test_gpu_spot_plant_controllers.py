"""The Spot controllers on perturbed plants (judo_amd/spot_plants.py) against plain `Controller`s on the single plants: an ensemble's member costs are the costs of a
plain controller on that member alone, its update is the ordinary update on the aggregated costs, and with identical members both controllers ARE a plain controller,
bit for bit, over plan steps that exercise the carried policy outputs and warm start.  No deadline (rollout_cutoff_time = None): timing cannot enter the results."""

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, H, TRACES = 6, 3, 2
SCALING = {
    "spot_box_push": dict(body_mass={"box_body": 1.7}, geom_friction={"box_collision": 0.6}, actuator_kp={None: 1.2}),
    "spot_navigate": dict(body_mass={"body": 1.7}, actuator_kp={None: 1.2}),
}


def _descs(task_name, M, identical=False):
    """M descriptions of the task's model: member 0 the task's own, the others scaled (each by its own factors), or all the task's own."""
    from judo_amd.models import scaled_description
    from judo_amd.tasks import get_registered_tasks

    base = get_registered_tasks()[task_name][0]().desc
    if identical:
        return [base] * M
    out = [base]
    for m in range(1, M):
        kw = {k: {name: 1.0 + (f - 1.0) / m for name, f in v.items()} for k, v in SCALING[task_name].items()}
        out.append(scaled_description(base, **kw))
    return out


def _plain(task_name, opt, desc):
    """A plain Controller that believes `desc`."""
    from judo_amd.controller import make_controller_for
    from judo_amd.models import layout
    from judo_amd.tasks import get_registered_tasks

    t = get_registered_tasks()[task_name][0]()
    t.desc = desc
    t._layout, t._ctrlrange, t._jadr, t._gpu = layout(desc), None, None, None
    return make_controller_for(t, opt)


def _state(task, step):
    rng = np.random.default_rng(50 + step)
    x = np.array(task.default_state(), dtype=np.float64)
    x[7:19] += 0.05 * rng.standard_normal(12)
    x[:2] += 0.1 * rng.standard_normal(2)
    if task.nq > 26:
        x[26:28] = [0.95, 0.0]  # the box within the arm's reach: its mass and friction matter
        x[26:28] += 0.02 * rng.standard_normal(2)
    return x


def _set_state(c, step):
    x = _state(c.task, step)
    c.update_states(x[: c.task.nq], x[c.task.nq :], 0.03 * step, {})


def _configure(c, opt, n=N, iters=1):
    c.optimizer.config.num_rollouts = n
    c.controller_cfg.horizon = H * c.task.dt
    c.controller_cfg.max_num_traces = TRACES
    c.controller_cfg.max_opt_iters = iters
    c.rollout_cutoff_time = None
    if opt == "cem":
        c.optimizer.sigma = ((c.optimizer.sigma_min + c.optimizer.sigma_max) / 2) * np.ones((c.optimizer.num_nodes, c.nu))
    np.random.seed(7)  # (Task.reset draws from numpy's global stream)
    c.reset()
    assert c.num_timesteps == H
    c.optimizer.seed(1234)
    goal = np.array(c.task.config.goal_position, dtype=np.float64)
    goal[:2] += [1.0, -0.3]
    c.task.config.goal_position = goal
    _set_state(c, 0)
    return c


def _snapshot(c):
    t = c.time + 0.5 * c.task.dt
    return dict(nominal=c.nominal_knots.copy(), times=np.array(c.times), traces=c.traces.copy(), rewards=np.array(c.rewards),
                sigma=np.atleast_1d(np.asarray(getattr(c.optimizer, "sigma", 0.0))).copy(), action=np.array(c.action(t)))


def _assert_same(a, b, what):
    for key in a:
        x, y = np.ascontiguousarray(a[key]), np.ascontiguousarray(b[key])
        assert x.shape == y.shape and x.dtype == y.dtype, (what, key, x.shape, y.shape)
        assert x.tobytes() == y.tobytes(), f"{what}: {key} differs (max |d| = {np.abs(x - y).max():.3e})"


def _costs(c):
    return c.costs_device.cpu().numpy()


def _ensemble(task_name, opt, descs, worst=None, **cfg):
    from judo_amd.spot_plants import make_spot_ensemble_controller

    return _configure(make_spot_ensemble_controller(task_name, opt, descs, worst=worst), opt, **cfg)


def _randomized(task_name, opt, descs, blocks=None, **cfg):
    from judo_amd.spot_plants import make_spot_randomized_controller

    return _configure(make_spot_randomized_controller(task_name, opt, descs, blocks=blocks), opt, **cfg)


@pytest.mark.parametrize("task_name,opt,worst", [("spot_box_push", "mppi", 1), ("spot_navigate", "cem", 2), ("spot_box_push", "ps", 2)])
def test_ensemble_member_costs_aggregation_and_update(gpu, task_name, opt, worst):
    """M = 3 different plants: member m's costs are a plain controller's on plant m; rewards are the negated host aggregation; nominal (and CEM's sigma) are what the
    ordinary update makes of those costs -- a plain controller whose rollout is replaced by them."""
    import torch

    from judo_amd.ensemble import aggregate_costs_host

    descs = _descs(task_name, 3)
    ens = _ensemble(task_name, opt, descs, worst=worst)
    assert ens.num_members == 3 and ens.worst == worst and ens.descriptions == descs
    ens.update_action()
    mc = ens.member_costs
    assert mc.shape == (3, N) and mc.dtype == np.float32
    for m in range(3):
        alone = _configure(_plain(task_name, opt, descs[m]), opt)
        alone.update_action()
        assert _costs(alone).tobytes() == mc[m].tobytes(), f"member {m}"
        if m == 0:  # member 0 is the nominal plant: last_rollout is its rows
            for x, y in zip(ens.last_rollout, alone.last_rollout):
                assert torch.equal(x, y)
    assert not np.array_equal(mc[0], mc[1]) and not np.array_equal(mc[1], mc[2])  # (identical costs would show nothing)
    agg = aggregate_costs_host(mc, worst)
    assert _costs(ens).tobytes() == agg.tobytes()
    assert np.array_equal(ens.rewards, -agg.astype(np.float64)) and np.array_equal(ens.member_rewards, -mc.astype(np.float64))
    fed = _configure(_plain(task_name, opt, descs[0]), opt)
    fed._materialised_costs = lambda *a, **k: torch.as_tensor(agg, device=fed.device)  # the ordinary jh_update_fused on the aggregated costs, same noise
    fed.update_action()
    assert fed.nominal_knots.tobytes() == ens.nominal_knots.tobytes()
    assert np.asarray(getattr(fed.optimizer, "sigma", 0.0)).tobytes() == np.asarray(getattr(ens.optimizer, "sigma", 0.0)).tobytes()
    st = ens.solver_stats()
    assert st["steps"] == 3 * N * H * ens.task.physics_substeps


@pytest.mark.parametrize("task_name,opt,M,worst,iters", [("spot_box_push", "mppi", 2, None, 1), ("spot_navigate", "cem", 3, 1, 1), ("spot_box_push", "ps", 2, 2, 2)])
def test_an_ensemble_of_identical_members_is_a_plain_controller(gpu, task_name, opt, M, worst, iters):
    """Three plan steps with new states in between (and max_opt_iters = 2 in one case): plan, traces, rewards, sigma and action equal a plain controller's, and every
    member's carried policy outputs and warm start equal the plain controller's own.  worst = 1 is the exact maximum; the mean of M = 2 equal values is exact."""
    descs = _descs(task_name, M, identical=True)
    ens, alone = _ensemble(task_name, opt, descs, worst=worst, iters=iters), _configure(_plain(task_name, opt, descs[0]), opt, iters=iters)
    for step in range(3):
        _set_state(ens, step)
        _set_state(alone, step)
        ens.update_action()
        alone.update_action()
        _assert_same(_snapshot(ens), _snapshot(alone), f"{task_name} {opt} step {step}")
        out, warm = alone._last_policy_output.cpu().numpy(), alone.rollout_backend._warm.cpu().numpy()
        assert np.abs(out).max() > 0 and np.abs(warm).max() > 0
        for m in range(M):
            rows = slice(m * N, (m + 1) * N)
            assert ens._plant_policy_out[rows].cpu().numpy().tobytes() == out.tobytes(), (step, m)
            assert ens._plant_backend._warm[rows].cpu().numpy().tobytes() == warm.tobytes(), (step, m)
    ens.reset()  # the carried state goes where the controller's own goes
    alone.reset()
    for c in (ens, alone):
        c.optimizer.seed(99)
        _set_state(c, 5)
        c.update_action()
    _assert_same(_snapshot(ens), _snapshot(alone), "after reset")


@pytest.mark.parametrize("task_name,opt", [("spot_box_push", "mppi"), ("spot_navigate", "ps")])
def test_randomized_blocks_run_on_their_plants(gpu, task_name, opt):
    """G = 2 blocks of 3 on plants [1, 0]: block g's costs are block g of a plain controller on plant assignment[g]; then the assignment is changed between plan steps."""
    descs = _descs(task_name, 2)
    rnd = _randomized(task_name, opt, descs, blocks=2)
    assert rnd.assignment == [0, 1] and rnd.blocks == 2 and rnd.num_members == 2
    rnd.assignment = [1, 0]
    assert rnd.plant_of_rollout.tolist() == [1, 1, 1, 0, 0, 0]
    rnd.update_action()
    got = _costs(rnd)
    alone = [_configure(_plain(task_name, opt, d), opt) for d in descs]
    for c in alone:
        c.update_action()
    ref = [_costs(c) for c in alone]
    assert not np.array_equal(ref[0], ref[1])
    assert got[:3].tobytes() == ref[1][:3].tobytes() and got[3:].tobytes() == ref[0][3:].tobytes()
    pr = rnd.plant_rewards()
    assert pr.shape == (2,) and pr[1] == np.mean(-got[:3].astype(np.float64)) and pr[0] == np.mean(-got[3:].astype(np.float64))
    st = rnd.solver_stats()
    assert st["steps"] == N * H * rnd.task.physics_substeps

    # all blocks on plant 0 from a fresh start is the plain controller on plant 0; the assignment changed for the next step moves block 0 alone
    rnd, p0 = _randomized(task_name, opt, descs, blocks=2), _configure(_plain(task_name, opt, descs[0]), opt)
    rnd.assignment = [0, 0]
    for c in (rnd, p0):
        c.update_action()
    _assert_same(_snapshot(rnd), _snapshot(p0), "assignment [0, 0]")
    rnd.assignment = [1, 0]
    for c in (rnd, p0):
        _set_state(c, 1)
        c.update_action()
    assert rnd.plant_of_rollout.tolist() == [1, 1, 1, 0, 0, 0]
    assert _costs(rnd)[3:].tobytes() == _costs(p0)[3:].tobytes() and not np.array_equal(_costs(rnd)[:3], _costs(p0)[:3])


@pytest.mark.parametrize("task_name,opt,G,iters", [("spot_box_push", "mppi", 3, 1), ("spot_navigate", "cem", 2, 2)])
def test_a_randomized_controller_on_identical_members_is_a_plain_controller(gpu, task_name, opt, G, iters):
    descs = _descs(task_name, 2, identical=True)
    rnd, alone = _randomized(task_name, opt, descs, blocks=G, iters=iters), _configure(_plain(task_name, opt, descs[0]), opt, iters=iters)
    for step in range(3):
        _set_state(rnd, step)
        _set_state(alone, step)
        rnd.update_action()
        alone.update_action()
        _assert_same(_snapshot(rnd), _snapshot(alone), f"{task_name} {opt} step {step}")
        assert rnd._last_policy_output.cpu().numpy().tobytes() == alone._last_policy_output.cpu().numpy().tobytes()
        assert rnd.rollout_backend._warm.cpu().numpy().tobytes() == alone.rollout_backend._warm.cpu().numpy().tobytes()


def test_set_member_and_a_live_change_of_num_rollouts(gpu):
    task_name, opt = "spot_box_push", "mppi"
    same, descs = _descs(task_name, 2, identical=True), _descs(task_name, 2)
    ens = _ensemble(task_name, opt, same)
    ens.set_member(1, descs[1])
    assert ens.descriptions[1] is descs[1]
    ens.update_action()
    for m in range(2):
        alone = _configure(_plain(task_name, opt, descs[m]), opt)
        alone.update_action()
        assert _costs(alone).tobytes() == ens.member_costs[m].tobytes(), f"member {m} after set_member"
    with pytest.raises(ValueError, match="member 2"):
        ens.set_member(2, descs[1])
    with pytest.raises(ValueError, match="worst = 3"):
        ens.worst = 3

    # a live change of num_rollouts: every carried row starts again from zero, as the plain controller's do
    ens, alone = _ensemble(task_name, opt, same), _configure(_plain(task_name, opt, same[0]), opt)
    rnd = _randomized(task_name, opt, same, blocks=2)
    for n in (N, 8):
        for c in (ens, alone, rnd):
            c.optimizer.config.num_rollouts = n
            _set_state(c, n)
            c.update_action()
        _assert_same(_snapshot(ens), _snapshot(alone), f"ensemble, {n} rollouts")
        _assert_same(_snapshot(rnd), _snapshot(alone), f"randomised, {n} rollouts")
        assert ens.member_costs.shape == (2, n) and ens._plant_policy_out.shape == (2 * n, 12)
    rnd.optimizer.config.num_rollouts = 7
    with pytest.raises(ValueError, match=r"num_rollouts % blocks != 0: 7 rollouts"):
        rnd.update_action()
    rnd.set_member(1, descs[1])
    rnd.optimizer.config.num_rollouts = N
    rnd.update_action()
    assert np.isfinite(rnd.rewards).all()


def test_fleets_and_the_sharded_path_refuse_the_new_classes(gpu):
    from judo_amd.ensemble_fleet import EnsembleFleet
    from judo_amd.fleet import ControllerFleet
    from judo_amd.randomized_fleet import RandomizedFleet

    descs = _descs("spot_navigate", 2, identical=True)
    ens, rnd = _ensemble("spot_navigate", "mppi", descs), _randomized("spot_navigate", "mppi", descs)
    for fleet in (ControllerFleet, EnsembleFleet, RandomizedFleet):
        for c in (ens, rnd):
            with pytest.raises(ValueError, match=rf"fleet member 0 is a {type(c).__name__}"):
                fleet([c])
    for c, kind in ((ens, "ensemble"), (rnd, "randomised")):
        c.force_shard_path = True
        with pytest.raises(ValueError, match=rf"the sharded path has no {kind} form"):
            c.update_action()


def test_one_plants_call_per_iteration(gpu, monkeypatch):
    """The rollouts of an iteration are ONE jh_policy_rollout_plants call -- never a jh_policy_rollout per member or per block."""
    from judo_amd import _lib

    L = _lib.lib()
    calls = {"plants": 0, "single": 0}
    plants, single = L.jh_policy_rollout_plants, L.jh_policy_rollout

    def count_plants(*a):
        calls["plants"] += 1
        return plants(*a)

    def count_single(*a):
        calls["single"] += 1
        return single(*a)

    descs = _descs("spot_box_push", 3)
    ens, rnd = _ensemble("spot_box_push", "mppi", descs, iters=2), _randomized("spot_box_push", "mppi", descs, blocks=3, iters=2)
    monkeypatch.setattr(L, "jh_policy_rollout_plants", count_plants)
    monkeypatch.setattr(L, "jh_policy_rollout", count_single)
    for c in (ens, rnd):
        calls.update(plants=0, single=0)
        c.update_action()
        assert calls == {"plants": 2, "single": 0}, (type(c).__name__, calls)
