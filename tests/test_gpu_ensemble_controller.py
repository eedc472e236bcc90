"""EnsembleController: one controller, one nominal, every candidate rolled out on M plants and scored by the mean of its `worst` largest member costs.

With identical members it is a plain controller, bit for bit; with distinct members its member costs are the costs plain controllers on the members' descriptions
compute from the same seed and state, its rewards the numpy restatement of the risk measure on them, and its plan another one than any member's own."""

import copy

import numpy as np
import pytest

from tests.test_gpu_model_set import CARTPOLE, LEAP_A, LEAP_B

pytestmark = pytest.mark.gpu

N, H, TRACES = 32, 8, 3


def _task(name):
    from judo_amd.tasks import get_registered_tasks

    return get_registered_tasks()[name][0]()


def _descriptions(name, perturbations):
    """The shipped description of `name` and one per perturbation (keyword arguments of models.scaled_description)."""
    from judo_amd.models import scaled_description

    desc = _task(name).desc
    return [copy.deepcopy(desc)] + [scaled_description(desc, **kw) for kw in perturbations]


def _plain_on(name, opt, desc):
    """A plain Controller whose task plans on `desc` (what make_controller_fleet does for a member with a description of its own)."""
    from judo_amd.controller import make_controller_for
    from judo_amd.models import layout

    t = _task(name)
    t.desc = desc
    t._layout, t._ctrlrange, t._jadr = layout(desc), None, None
    return make_controller_for(t, opt)


def _configure(c, opt, seed=5):
    c.optimizer.config.num_rollouts = N
    c.controller_cfg.horizon = H * c.task.dt
    c.controller_cfg.max_num_traces = TRACES
    if opt == "cem":
        c.optimizer.sigma = ((c.optimizer.sigma_min + c.optimizer.sigma_max) / 2) * np.ones((c.optimizer.num_nodes, c.nu))
    np.random.seed(100 + seed)  # (Task.reset draws the start state from numpy's global stream)
    c.reset()
    assert c.num_timesteps == H
    c.optimizer.seed(1000 + seed)
    _set_state(c, 0)


def _set_state(c, step):
    rng = np.random.default_rng(step)
    x = c.task.default_state() + 0.02 * rng.standard_normal(c.task.nq + c.task.nv)
    meta = {}
    if c.task.name == "leap_cube":
        q = rng.standard_normal(4)
        meta = {"goal_quat": q / np.linalg.norm(q)}
    c.update_states(x[: c.task.nq], x[c.task.nq :], 0.03 * step, meta)


def _same(x, y, what):
    x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
    assert x.shape == y.shape and x.dtype == y.dtype, what
    assert x.tobytes() == y.tobytes(), f"{what} differs (max |d| = {np.abs(x - y).max():.3e})"


@pytest.mark.parametrize("M,worst", [(2, None), (3, 1)])
@pytest.mark.parametrize("task,opt", [("cartpole", "mppi"), ("cartpole", "cem"), ("leap_cube", "mppi")])
def test_identical_members_match_a_plain_controller(gpu, task, opt, M, worst):
    """M identical descriptions: the maximum of equal costs is the cost and (c + c) / 2 is exact, so three plan steps in closed sequence from the same seed leave
    nominal_knots, rewards and traces where make_controller's controller leaves them, bit for bit.

    The traces: an ensemble launch writes no trace buffer, its elites are re-rolled on member 0.  A plain controller by default gathers the fused kernel's own trace rows
    instead, and the fused and the materialise instantiation of a kernel round differently in the last bits (tests/test_gpu_controller.py::
    test_traces_from_the_fused_kernel_equal_the_re_rolled_elites, atol 2e-5).  So the traces are compared bit for bit with a plain controller that re-rolls as well
    (`fused_traces = False`: the same plan, as that test shows) and at that test's bound with the default one; nominal_knots and rewards bit for bit with both."""
    from judo_amd.controller import make_controller
    from judo_amd.ensemble import EnsembleController, make_ensemble_controller

    desc = _task(task).desc
    ens = make_ensemble_controller(task, opt, [copy.deepcopy(desc) for _ in range(M)], worst=worst)
    assert isinstance(ens, EnsembleController) and ens.worst == (M if worst is None else worst) and ens.num_members == M and len(ens.descriptions) == M
    plain, rerolled = make_controller(task, opt), make_controller(task, opt)
    rerolled.fused_traces = False
    for c in (ens, plain, rerolled):
        _configure(c, opt)
    for step in range(3):
        for c in (ens, plain, rerolled):
            _set_state(c, step)
            c.update_action()
        for other, name in ((plain, "the default controller"), (rerolled, "the re-rolling controller")):
            _same(ens.nominal_knots, other.nominal_knots, f"{task} {opt} step {step}: nominal_knots against {name}")
            _same(ens.rewards, other.rewards, f"{task} {opt} step {step}: rewards against {name}")
        _same(ens.traces, rerolled.traces, f"{task} {opt} step {step}: traces")
        assert ens.traces.shape == plain.traces.shape == (TRACES * len(ens.trace_sensors) * (H - 1), 2, 3)
        d = float(np.abs(ens.traces - plain.traces).max())
        print(f"{task} {opt} step {step}: max |traces - fused-kernel traces| = {d:.3e}")
        np.testing.assert_allclose(ens.traces, plain.traces, rtol=0, atol=2e-5)
        mc = ens.member_costs
        assert mc.shape == (M, N) and all(mc[b].tobytes() == mc[0].tobytes() for b in range(M))
        _same(ens.member_rewards[0], plain.rewards, "member_rewards")


@pytest.mark.parametrize("task,opt,pert,worst", [("cartpole", "mppi", CARTPOLE, 2), ("cartpole", "cem", CARTPOLE, 1), ("leap_cube", "mppi", [LEAP_A, LEAP_B], None)])
def test_distinct_members_first_plan_step(gpu, task, opt, pert, worst):
    """M = 3 distinct descriptions, the first plan step from one seed and state: member b's costs are the costs of a plain controller on descriptions[b], the rewards the
    negated numpy restatement of the risk measure on them, and the MPPI plan differs from every member's own."""
    from judo_amd.ensemble import aggregate_costs_host, make_ensemble_controller

    descs = _descriptions(task, pert)
    ens = make_ensemble_controller(task, opt, descs, worst=worst)
    plains = [_plain_on(task, opt, d) for d in descs]
    for c in [ens] + plains:
        _configure(c, opt)
        c.update_action()
    mc = ens.member_costs
    assert mc.shape == (3, N) and mc.dtype == np.float32
    for b, p in enumerate(plains):
        _same(-mc[b].astype(np.float64), p.rewards, f"{task} {opt}: member {b}'s costs against a plain controller on its description")
        _same(ens.member_rewards[b], p.rewards, f"member_rewards[{b}]")
        if opt == "mppi":  # (every cost enters the MPPI weights; the CEM / PS nominal is a function of the elite SET alone, which two cost vectors may share)
            assert (ens.nominal_knots != p.nominal_knots).any(), b
    assert len({mc[b].tobytes() for b in range(3)}) == 3
    _same(ens.rewards, -aggregate_costs_host(mc, ens.worst).astype(np.float64), f"{task} {opt}: rewards")
    assert np.isfinite(ens.nominal_knots).all() and ens.traces.shape[0] == TRACES * len(ens.trace_sensors) * (H - 1)
    assert ens.model is ens.model_set.models[0] and ens.model.desc is descs[0]  # member 0 is the nominal plant


def test_one_library_call_per_iteration(gpu, monkeypatch):
    """update_action() is one jh_plan_step_ensemble per optimiser iteration and no jh_plan_step, counted on the bound symbols."""
    from judo_amd import _lib
    from judo_amd.ensemble import make_ensemble_controller

    L = _lib.lib()
    calls = {"jh_plan_step_ensemble": 0, "jh_plan_step": 0, "jh_plan_step_batch_models": 0, "jh_update_fused": 0, "jh_rollout_cost_traced": 0}

    def counted(name):
        fn = getattr(L, name)

        def wrapper(*a):
            calls[name] += 1
            return fn(*a)

        return wrapper

    for name in calls:
        monkeypatch.setattr(L, name, counted(name))
    ens = make_ensemble_controller("cartpole", "cem", _descriptions("cartpole", CARTPOLE))
    _configure(ens, "cem")
    ens.controller_cfg.max_opt_iters = 2
    ens.update_action()
    assert calls == {"jh_plan_step_ensemble": 2, "jh_plan_step": 0, "jh_plan_step_batch_models": 0, "jh_update_fused": 0, "jh_rollout_cost_traced": 0}
    ens.optimizer.config.num_rollouts = 2 * N  # a live change of num_rollouts
    _set_state(ens, 1)
    ens.update_action()
    assert calls["jh_plan_step_ensemble"] == 4 and calls["jh_plan_step"] == 0
    assert ens.member_costs.shape == (3, 2 * N) and ens.rewards.shape == (2 * N,) and np.isfinite(ens.nominal_knots).all()


def test_member_and_worst_changes_between_plan_steps(gpu):
    """Two ensembles in lockstep.  After `set_member(1, ...)` on one of them the next plan step differs in member 1's costs -- in every rollout -- and in nothing else
    that does not follow from them; `worst` set between steps is the risk measure of the next step."""
    from judo_amd.ensemble import aggregate_costs_host, make_ensemble_controller
    from judo_amd.models import scaled_description

    descs = _descriptions("cartpole", CARTPOLE)
    a, b = make_ensemble_controller("cartpole", "mppi", descs), make_ensemble_controller("cartpole", "mppi", descs)
    for c in (a, b):
        _configure(c, "mppi")
        c.update_action()
    _same(a.nominal_knots, b.nominal_knots, "step 0")
    new = scaled_description(descs[0], body_mass={"pole": 2.0, "cart": 0.8})
    a.set_member(1, new)
    assert a.descriptions[1] is new and a.descriptions[0] is descs[0] and a.model_set.info()["distinct_from_first"] == 2
    for c in (a, b):
        _set_state(c, 1)
        c.update_action()
    ma, mb = a.member_costs, b.member_costs
    assert ma[0].tobytes() == mb[0].tobytes() and ma[2].tobytes() == mb[2].tobytes()
    assert (ma[1] != mb[1]).all()  # every rollout of member 1 ran on another plant
    _same(a.rewards, -aggregate_costs_host(ma, 3).astype(np.float64), "rewards after set_member")
    b.worst = 1
    assert b.worst == 1
    _set_state(b, 2)
    b.update_action()
    mb = b.member_costs
    _same(b.rewards, -aggregate_costs_host(mb, 1).astype(np.float64), "rewards after worst = 1")
    assert (b.rewards != -aggregate_costs_host(mb, 3).astype(np.float64)).any()
    for bad in (0, 4):
        with pytest.raises(ValueError, match="worst"):
            b.worst = bad
    with pytest.raises(ValueError, match="member 3"):
        b.set_member(3, new)
    assert b.model_set.info()["distinct_from_first"] == 2  # (a refused change leaves the set as it was)


def test_configurations_without_a_one_call_iteration_are_refused(gpu):
    """Every configuration whose iteration is not the one-call shape raises ValueError naming the reason, before anything is launched."""
    from judo_amd.ensemble import make_ensemble_controller

    descs = _descriptions("cartpole", CARTPOLE)

    def fresh(task="cartpole"):
        c = make_ensemble_controller(task, "mppi", descs)
        _configure(c, "mppi")
        return c

    c = fresh()
    c.force_shard_path = True
    with pytest.raises(ValueError, match="force_shard_path"):
        c.update_action()
    c.force_shard_path = False
    c.controller_cfg.action_normalizer = "running"
    with pytest.raises(ValueError, match="running normaliser"):
        c.update_action()
    c.controller_cfg.action_normalizer = "none"
    c.keep_candidates = True
    with pytest.raises(ValueError, match="keep_candidates"):
        c.update_action()
    c.keep_candidates = False
    K = c.optimizer.config.num_nodes
    c.optimizer.config.num_nodes = c.model.max_fused_knots_at(H) + 1
    assert c.optimizer.config.num_nodes * c.nu <= 512
    with pytest.raises(ValueError, match="max_fused_knots_at"):
        c.update_action()
    c.optimizer.config.num_nodes = K
    c.reset()
    c.update_action()  # (and the controller plans again once the configuration is the one-call shape)
    assert np.isfinite(c.nominal_knots).all()

    base = type(_task("cartpole"))

    class Hooked(base):  # a plugin task that keeps the shipped reward but overrides a hook: the materialise path
        def post_rollout(self, *args, **kwargs):
            return None

    hooked = fresh(Hooked())
    assert not hooked.uses_fused_cost
    with pytest.raises(ValueError, match="uses_fused_cost"):
        hooked.update_action()
    c.controller_cfg.action_normalizer = "min_max"  # (the min_max normaliser is affine and needs no moments: it plans)
    c.update_action()
    assert np.isfinite(c.nominal_knots).all()
    with pytest.raises(ValueError, match="fr3_pick"):
        make_ensemble_controller("fr3_pick", "cem", [_task("fr3_pick").desc])
    with pytest.raises(ValueError, match="Spot policy"):
        make_ensemble_controller("spot_navigate", "mppi", [_task("spot_navigate").desc])
    with pytest.raises(ValueError, match="int section|header|float section"):
        make_ensemble_controller("cartpole", "mppi", [descs[0], _task("cylinder_push").desc])
