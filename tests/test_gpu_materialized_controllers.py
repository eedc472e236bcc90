"""MaterializedEnsembleController and MaterializedRandomizedController (judo_amd/materialized.py) against plain `Controller`s on the materialise path: with identical
members both ARE a plain controller with `force_materialize`, bit for bit, over plan steps and under the running normaliser; with distinct plants an ensemble's member
costs are the costs of a plain materialise controller on that plant, its rewards the host restatement of the risk measure, and a randomised controller's block g is
block g of the plain controller on plant `assignment[g]`.  Plugin rewards, hooks and optimizers -- what the fused classes refuse -- plan.  Everything compared is
compared bit for bit."""

import copy

import numpy as np
import pytest

from tests import plugin_fixture as PF
from tests.test_gpu_ensemble_controller import _descriptions, _plain_on, _same, _set_state, _task
from tests.test_gpu_model_set import CARTPOLE, LEAP_A, LEAP_C

pytestmark = pytest.mark.gpu

N, TRACES = 32, 3
HORIZON = {"cartpole": 25, "leap_cube": 8}
PERT = {"cartpole": CARTPOLE, "leap_cube": [LEAP_A, LEAP_C]}


def _configure(c, opt, normalizer="none", seed=5):
    H = HORIZON[c.task.desc.get("family", c.task.desc["task"])]
    c.optimizer.config.num_rollouts = N
    c.controller_cfg.horizon = H * c.task.dt
    c.controller_cfg.max_num_traces = TRACES
    c.controller_cfg.action_normalizer = normalizer
    if opt == "cem":
        c.optimizer.sigma = ((c.optimizer.sigma_min + c.optimizer.sigma_max) / 2) * np.ones((c.optimizer.num_nodes, c.nu))
    np.random.seed(100 + seed)  # (Task.reset draws the start state from numpy's global stream)
    c.reset()
    assert c.num_timesteps == H
    if hasattr(c.optimizer, "seed"):
        c.optimizer.seed(1000 + seed)
    _set_state(c, 0)
    return c


def _plain(task, opt, desc=None, **kw):
    """A plain Controller on the materialise path (`force_materialize`), on the task's own description or on `desc`."""
    from judo_amd.controller import make_controller_for

    c = make_controller_for(task if not isinstance(task, str) else _task(task), opt) if desc is None else _plain_on(task, opt, desc)
    c.force_materialize = True
    return _configure(c, opt, **kw)


def _ensemble(task, opt, descs, worst=None, **kw):
    from judo_amd.materialized import make_materialized_ensemble_controller

    return _configure(make_materialized_ensemble_controller(task, opt, descs, worst=worst), opt, **kw)


def _randomized(task, opt, descs, blocks=None, **kw):
    from judo_amd.materialized import make_materialized_randomized_controller

    return _configure(make_materialized_randomized_controller(task, opt, descs, blocks=blocks), opt, **kw)


def _costs(c):
    return c.costs_device.cpu().numpy()


def _snapshot(c):
    return dict(nominal=c.nominal_knots.copy(), rewards=np.array(c.rewards), traces=c.traces.copy(), sigma=np.atleast_1d(np.asarray(getattr(c.optimizer, "sigma", 0.0))).copy(),
                action=np.array(c.action(c.time + 0.5 * c.task.dt)))


def _assert_same(a, b, what):
    for key in a:
        _same(a[key], b[key], f"{what}: {key}")


@pytest.mark.parametrize("normalizer", ["none", "running"])
@pytest.mark.parametrize("task,opt", [(t, o) for t in ("cartpole", "leap_cube") for o in ("mppi", "cem", "ps")])
def test_identical_members_are_a_plain_materialise_controller(gpu, task, opt, normalizer):
    """M = 3 identical members, three plan steps with new states in between: nominal knots, rewards, traces (and CEM's sigma, the action) of both new controllers equal
    a plain controller's with `force_materialize`, with and without the running normaliser.  The ensemble takes worst = 1, the exact maximum of three equal costs (their
    mean, (c + c + c) / 3 in fp32, is not always c); the randomised controller 4 blocks of 8 on plants [0, 1, 2, 0]."""
    from judo_amd.materialized import MaterializedEnsembleController, MaterializedRandomizedController

    descs = [copy.deepcopy(_task(task).desc) for _ in range(3)]
    ens, rnd, alone = _ensemble(task, opt, descs, worst=1, normalizer=normalizer), _randomized(task, opt, descs, blocks=4, normalizer=normalizer), _plain(task, opt, normalizer=normalizer)
    assert isinstance(ens, MaterializedEnsembleController) and isinstance(rnd, MaterializedRandomizedController)
    assert ens.num_members == rnd.num_members == 3 and rnd.assignment == [0, 1, 2, 0] and not ens.uses_fused_cost and not rnd.uses_fused_cost and not alone.uses_fused_cost
    assert alone._iteration_shape(1, alone._current_normalizer()) == ens._iteration_shape(1, ens._current_normalizer()) == "update_fused"
    for step in range(3):
        for c in (ens, rnd, alone):
            _set_state(c, step)
            c.update_action()
        want = _snapshot(alone)
        assert want["traces"].shape == (TRACES * len(alone.trace_sensors) * (alone.num_timesteps - 1), 2, 3)
        _assert_same(_snapshot(ens), want, f"ensemble, {task} {opt} {normalizer} step {step}")
        _assert_same(_snapshot(rnd), want, f"randomised, {task} {opt} {normalizer} step {step}")
        mc = ens.member_costs
        assert mc.shape == (3, N) and all(mc[m].tobytes() == _costs(alone).tobytes() for m in range(3))
    if normalizer == "running":
        assert np.array_equal(ens.action_normalizer.mean, alone.action_normalizer.mean) and np.array_equal(rnd.action_normalizer.std, alone.action_normalizer.std)


@pytest.mark.parametrize("task,opt", [("cartpole", "mppi"), ("cartpole", "cem"), ("leap_cube", "ps")])
def test_distinct_plants_member_costs_and_aggregation(gpu, task, opt):
    """M = 3 distinct plants, the first plan step from one seed and state: member m's costs are the costs of a plain materialise controller on plant m (and member 0's
    rows are `last_rollout`); the rewards the negated host restatement of the risk measure for worst = 1, 2 and M."""
    import torch

    from judo_amd.ensemble import aggregate_costs_host

    descs = _descriptions(task, PERT[task])
    plains = [_plain(task, opt, d) for d in descs]
    for c in plains:
        c.update_action()
    ref = np.stack([_costs(c) for c in plains])
    assert not np.array_equal(ref[0], ref[1]) and not np.array_equal(ref[1], ref[2]) and not np.array_equal(ref[0], ref[2])  # (identical costs would show nothing)
    for worst in (1, 2, 3):
        ens = _ensemble(task, opt, descs, worst=worst)
        assert ens.worst == worst and ens.descriptions == descs
        ens.update_action()
        mc = ens.member_costs
        assert mc.shape == (3, N) and mc.dtype == np.float32
        for m in range(3):
            _same(mc[m], ref[m], f"{task} {opt}: member_costs[{m}] against the plain controller on plant {m}")
        agg = aggregate_costs_host(mc, worst)
        _same(_costs(ens), agg, f"worst = {worst}: aggregated costs")
        assert np.array_equal(ens.rewards, -agg.astype(np.float64)) and np.array_equal(ens.member_rewards, -mc.astype(np.float64))
        for x, y in zip(ens.last_rollout, plains[0].last_rollout):  # member 0 is the nominal plant
            assert torch.equal(x, y)
        if worst == 1:  # the update is the ordinary one on the aggregated costs: a plain controller whose rollout is replaced by them
            fed = _plain(task, opt, descs[0])
            fed._materialised_costs = lambda *a, **k: torch.as_tensor(agg, device=fed.device)
            fed.update_action()
            _same(fed.nominal_knots, ens.nominal_knots, "nominal_knots against the update on the aggregated costs")


@pytest.mark.parametrize("task,opt", [("cartpole", "mppi"), ("leap_cube", "mppi")])
def test_randomized_blocks_run_on_their_plants(gpu, task, opt):
    """G = 4 blocks of 8.  First plan step, assignment [2, 0, 1, 0]: block g is rows [8 g, 8 g + 8) of the plain materialise controller on plant assignment[g].  Then,
    from a first step with every block on plant 0 (the plain controller on plant 0, whose costs the plain controllers on plants 1 and 2 are fed so that all four stand
    at the same nominal, noise stream and state), the assignment is re-set to [1, 0, 2, 0] and the second step's blocks follow it."""
    import torch

    descs, n = _descriptions(task, PERT[task]), N // 4
    rnd = _randomized(task, opt, descs, blocks=4)
    assert rnd.assignment == [0, 1, 2, 0] and rnd.blocks == 4
    rnd.assignment = [2, 0, 1, 0]
    assert rnd.plant_of_rollout.tolist() == [2] * n + [0] * n + [1] * n + [0] * n
    rnd.update_action()
    plains = [_plain(task, opt, d) for d in descs]
    for c in plains:
        c.update_action()
    ref, got = [_costs(c) for c in plains], _costs(rnd)
    assert all(not np.array_equal(ref[a], ref[b]) for a, b in ((0, 1), (1, 2), (0, 2)))
    for g, p in enumerate([2, 0, 1, 0]):
        _same(got[g * n : (g + 1) * n], ref[p][g * n : (g + 1) * n], f"{task}: block {g} on plant {p}")
    pr = rnd.plant_rewards()
    assert pr.shape == (3,) and pr[2] == np.mean(-got[:n].astype(np.float64)) and pr[0] == np.mean(-np.concatenate([got[n : 2 * n], got[3 * n :]]).astype(np.float64))

    rnd, plains = _randomized(task, opt, descs, blocks=4), [_plain(task, opt, d) for d in descs]
    rnd.assignment = [0, 0, 0, 0]
    rnd.update_action()
    plains[0].update_action()
    _assert_same(_snapshot(rnd), _snapshot(plains[0]), "every block on plant 0")
    first = _costs(plains[0]).copy()
    for c in plains[1:]:
        own = c._materialised_costs
        c._materialised_costs = lambda *a, **k: torch.as_tensor(first, device=c.device)
        c.update_action()
        c._materialised_costs = own
        _same(c.nominal_knots, plains[0].nominal_knots, "the fed controllers stand where plant 0's stands")
    rnd.assignment = [1, 0, 2, 0]
    for c in [rnd] + plains:
        _set_state(c, 1)
        c.update_action()
    assert rnd.plant_of_rollout.tolist() == [1] * n + [0] * n + [2] * n + [0] * n
    ref, got = [_costs(c) for c in plains], _costs(rnd)
    for g, p in enumerate([1, 0, 2, 0]):
        _same(got[g * n : (g + 1) * n], ref[p][g * n : (g + 1) * n], f"{task}: second step, block {g} on plant {p}")
    assert not np.array_equal(got[:n], ref[0][:n]) and not np.array_equal(got[2 * n : 3 * n], ref[0][2 * n : 3 * n])


def _plugin_leap_task():
    """A third-party task on the leap_cube model: a torch reward of its own (keep the cube where it is, with a small control penalty) and a `post_rollout` that counts its
    calls and the rows it was given."""
    import torch

    base = type(_task("leap_cube"))

    class CubeKeeper(base):
        def __init__(self):
            super().__init__()
            self.hook_rows = []

        def post_rollout(self, states, sensors, controls, system_metadata=None):
            assert states.is_cuda and sensors.is_cuda and controls.is_cuda
            self.hook_rows.append((int(states.shape[0]), int(sensors.shape[0]), int(controls.shape[0])))

        def reward(self, states, sensors, controls, system_metadata=None):
            assert torch.is_tensor(states) and states.is_cuda
            target = torch.tensor([0.0, 0.03, 0.1], dtype=states.dtype, device=states.device)
            d = states[..., :3] - target
            return -((d * d).sum(-1).sum(-1) + 1e-3 * (controls * controls).sum(-1).sum(-1))

    return CubeKeeper()


def test_a_plugin_task_plans_on_the_plants(gpu):
    """A task with a torch reward of its own and a counting post_rollout: both controllers plan; the hook ran M times per iteration for the ensemble, on N rows each, and
    once for the randomised controller; the rewards are the plugin's, recomputed here from the materialised rollouts."""
    import torch

    from judo_amd.ensemble import aggregate_costs_host, make_ensemble_controller

    descs = _descriptions("leap_cube", PERT["leap_cube"])
    ens, rnd = _ensemble(_plugin_leap_task(), "mppi", descs, worst=2), _randomized(_plugin_leap_task(), "mppi", descs, blocks=4)
    for c in (ens, rnd):
        c.controller_cfg.max_opt_iters = 2
        before = c.nominal_knots.copy()
        c.update_action()
        assert np.isfinite(c.nominal_knots).all() and not np.array_equal(c.nominal_knots, before) and c.traces.shape[1:] == (2, 3)
    assert ens.task.hook_rows == [(N, N, N)] * (3 * 2) and rnd.task.hook_rows == [(N, N, N)] * 2
    states, sensors, controls = rnd.last_rollout
    assert tuple(states.shape) == (N, HORIZON["leap_cube"], rnd.model.nx)
    want = rnd.task.reward(states, sensors, controls, rnd.system_metadata).to(torch.float32)
    assert torch.equal(-rnd.costs_device, want) and np.array_equal(rnd.rewards, want.cpu().numpy().astype(np.float64))
    states, sensors, controls = ens.last_rollout  # member 0's rows
    want0 = ens.task.reward(states, sensors, controls, ens.system_metadata).to(torch.float32).cpu().numpy()
    mc = ens.member_costs
    assert np.array_equal(-mc[0], want0) and not np.array_equal(mc[0], mc[1]) and not np.array_equal(mc[1], mc[2])
    assert np.array_equal(ens.rewards, -aggregate_costs_host(mc, 2).astype(np.float64))
    # ... which the fused class refuses, naming the maker that serves it
    fused = _configure(make_ensemble_controller(_plugin_leap_task(), "mppi", descs), "mppi")
    with pytest.raises(ValueError, match=r"uses_fused_cost is false\): the members' costs come from the fused kernels alone.*make_materialized_ensemble_controller"):
        fused.update_action()


class _NumpyRewardCartpole:
    """Mixed into the cartpole task below: a numpy-only reward (one host round trip of the trajectories)."""

    reward_accepts_torch = False

    def reward(self, states, sensors, controls, system_metadata=None):
        assert isinstance(states, np.ndarray) and states.dtype == np.float64
        return PF.reward_numpy(states, sensors, controls)


def _numpy_task():
    base = type(_task("cartpole"))
    return type("NumpyRewardCartpole", (_NumpyRewardCartpole, base), {})()


def _plugin_optimizer(nu):
    from judo_amd.config import OptimizerConfig
    from judo_amd.optimizers import Optimizer

    class BestOfRandom(Optimizer):  # only the reference's two numpy methods: the candidates iteration
        def sample_control_knots(self, nominal_knots):
            noise = 0.3 * np.random.randn(self.num_rollouts, self.config.num_nodes, self.nu)
            noise[0] = 0.0
            return nominal_knots + noise

        def update_nominal_knots(self, sampled_knots, rewards):
            return sampled_knots[int(np.argmax(rewards))]

    return BestOfRandom(OptimizerConfig(), nu)


@pytest.mark.parametrize("plugin_optimizer", [False, True], ids=["fused_optimizer", "plugin_optimizer"])
def test_numpy_rewards_and_plugin_optimizers_equal_the_plain_controller(gpu, plugin_optimizer):
    """A numpy-only plugin reward, with MPPI and with a plugin optimizer that has the reference's two numpy methods alone: with identical members both new controllers equal
    the plain controller, three plan steps."""
    descs = [copy.deepcopy(_task("cartpole").desc) for _ in range(3)]
    ens, rnd, alone = _ensemble(_numpy_task(), "mppi", descs, worst=1), _randomized(_numpy_task(), "mppi", descs, blocks=2), _plain(_numpy_task(), "mppi")
    if plugin_optimizer:
        for c in (ens, rnd, alone):
            c.optimizer = _plugin_optimizer(c.nu)
            _configure(c, "plugin")
            assert not c.uses_fused_optimizer
    for step in range(3):
        for c in (ens, rnd, alone):
            np.random.seed(77 + step)  # (the plugin optimizer draws from numpy's global stream)
            _set_state(c, step)
            c.update_action()
        want = _snapshot(alone)
        assert np.isfinite(want["nominal"]).all() and np.abs(want["rewards"]).max() > 0
        _assert_same(_snapshot(ens), want, f"ensemble step {step}")
        _assert_same(_snapshot(rnd), want, f"randomised step {step}")
        _same(ens.candidate_knots, alone.candidate_knots, "candidate_knots")


def test_a_live_num_nodes_edit_above_the_fused_limit_plans(gpu):
    """num_nodes above max_fused_knots_at(H): the new controllers plan (and equal the plain controller, which takes the materialise path there by itself); the fused
    EnsembleController raises."""
    from judo_amd.ensemble import make_ensemble_controller

    descs = _descriptions("cartpole", CARTPOLE)
    same = [descs[0]] * 3
    ens, rnd, alone, fused = _ensemble("cartpole", "mppi", same, worst=1), _randomized("cartpole", "mppi", same, blocks=4), _plain("cartpole", "mppi"), make_ensemble_controller("cartpole", "mppi", descs)
    _configure(fused, "mppi")
    for c in (ens, rnd, alone, fused):
        c.update_action()
    K = alone.model.max_fused_knots_at(HORIZON["cartpole"]) + 1
    assert K * alone.nu <= 512
    for c in (ens, rnd, alone, fused):
        c.optimizer.config.num_nodes = K
        _set_state(c, 1)
    with pytest.raises(ValueError, match=r"max_fused_knots_at.*make_materialized_ensemble_controller"):
        fused.update_action()
    for c in (ens, rnd, alone):
        c.update_action()
        assert c.nominal_knots.shape == (K, 1) and np.isfinite(c.nominal_knots).all()
    _assert_same(_snapshot(ens), _snapshot(alone), "ensemble at K above the fused limit")
    _assert_same(_snapshot(rnd), _snapshot(alone), "randomised at K above the fused limit")
    distinct = _ensemble("cartpole", "mppi", descs)
    distinct.optimizer.config.num_nodes = K
    distinct.update_action()
    mc = distinct.member_costs
    assert np.isfinite(mc).all() and not np.array_equal(mc[0], mc[1])


def test_set_member_live_rollouts_and_refusals(gpu):
    descs = _descriptions("cartpole", CARTPOLE)
    ens = _ensemble("cartpole", "mppi", [descs[0]] * 3)
    ens.set_member(1, descs[1])
    ens.set_member(2, descs[2])
    assert ens.descriptions[1] is descs[1] and ens.model_set.info()["distinct_from_first"] == 2
    ens.update_action()
    for m in range(3):
        alone = _plain("cartpole", "mppi", descs[m])
        alone.update_action()
        _same(ens.member_costs[m], _costs(alone), f"member {m} after set_member")
    with pytest.raises(ValueError, match="member 3"):
        ens.set_member(3, descs[1])
    with pytest.raises(ValueError, match="worst = 4"):
        ens.worst = 4
    rnd = _randomized("cartpole", "mppi", descs, blocks=4)
    rnd.set_weights([0, 1, 1])
    assert rnd.assignment == [1, 1, 2, 2]
    with pytest.raises(ValueError, match=r"assignment\[0\] = 3"):
        rnd.assignment = [3, 0]
    rnd.optimizer.config.num_rollouts = 30
    with pytest.raises(ValueError, match=r"num_rollouts % blocks != 0: 30 rollouts"):
        rnd.update_action()
    rnd.optimizer.config.num_rollouts = 36  # a live change of num_rollouts: blocks of 9
    rnd.update_action()
    assert rnd.rewards.shape == (36,) and np.isfinite(rnd.rewards).all() and rnd.plant_of_rollout.tolist() == [1] * 18 + [2] * 18
    for c, kind in ((ens, "ensemble"), (rnd, "randomised")):
        c.force_shard_path = True
        with pytest.raises(ValueError, match=rf"the sharded path has no {kind} form"):
            c.update_action()
        c.force_shard_path = False


def test_one_plants_call_per_iteration(gpu, monkeypatch):
    """The rollouts of an iteration are ONE jh_rollout_materialize_plants call -- never a jh_rollout_materialize per member or per block -- and one jh_spline_controls."""
    from judo_amd import _lib

    L = _lib.lib()
    calls = {"plants": 0, "single": 0, "spline": 0}
    shapes = []
    plants, single, spline = L.jh_rollout_materialize_plants, L.jh_rollout_materialize, L.jh_spline_controls

    def count_plants(*a):
        calls["plants"] += 1
        shapes.append((a[2], a[3], a[7]))  # G, n, controls_shared
        return plants(*a)

    def count_single(*a):
        calls["single"] += 1
        return single(*a)

    def count_spline(*a):
        calls["spline"] += 1
        return spline(*a)

    descs = _descriptions("cartpole", CARTPOLE)
    ens, rnd = _ensemble("cartpole", "mppi", descs), _randomized("cartpole", "mppi", descs, blocks=4)
    for c in (ens, rnd):
        c.controller_cfg.max_opt_iters = 2
        c.controller_cfg.max_num_traces = 0  # (no traces: nothing is re-rolled behind the plan step)
    monkeypatch.setattr(L, "jh_rollout_materialize_plants", count_plants)
    monkeypatch.setattr(L, "jh_rollout_materialize", count_single)
    monkeypatch.setattr(L, "jh_spline_controls", count_spline)
    for c, shape in ((ens, (3, N, 1)), (rnd, (4, N // 4, 0))):
        calls.update(plants=0, single=0, spline=0)
        del shapes[:]
        c.update_action()
        assert calls == {"plants": 2, "single": 0, "spline": 2} and shapes == [shape] * 2, (type(c).__name__, calls, shapes)
