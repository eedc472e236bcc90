"""RandomizedController: one controller, one nominal, rollout block g of its candidates on plant assignment[g] of a model set, the update on the N costs as they are.

With identical members it is a plain controller, bit for bit; with distinct members block g of its rewards is that block of a plain controller on plant
assignment[g]'s description from the same seed and state, and its nominal is jh_update_fused on those rewards with its own block and noise.  No tolerance anywhere."""

import copy

import numpy as np
import pytest

from tests.test_gpu_ensemble_controller import _descriptions, _plain_on, _same, _set_state, _task
from tests.test_gpu_model_set import CARTPOLE, LEAP_A, LEAP_B

pytestmark = pytest.mark.gpu

N, H, TRACES = 48, 8, 3  # (48 rollouts: blocks of 16, 12 and 8 for G = 3, 4 and 6)


def _configure(c, opt, seed=5, n=N):
    c.optimizer.config.num_rollouts = n
    c.controller_cfg.horizon = H * c.task.dt
    c.controller_cfg.max_num_traces = TRACES
    c.controller_cfg.max_opt_iters = 1
    if opt == "cem":
        c.optimizer.sigma = ((c.optimizer.sigma_min + c.optimizer.sigma_max) / 2) * np.ones((c.optimizer.num_nodes, c.nu))
    np.random.seed(100 + seed)  # (Task.reset draws the start state from numpy's global stream)
    c.reset()
    assert c.num_timesteps == H
    c.optimizer.seed(1000 + seed)
    _set_state(c, 0)


def _stitch(plains, a, n=N):
    """Block g of the rewards of the plain controller on plant a[g]."""
    nb = n // len(a)
    return np.concatenate([plains[p].rewards[g * nb : (g + 1) * nb] for g, p in enumerate(a)])


def _update_fused(c, rewards):
    """nominal (K, nu) fp64 of jh_update_fused on the costs -rewards with the block and the noise of c's last plan step (the identity normaliser: raw units)."""
    import torch

    from judo_amd import _lib

    L = _lib.lib()
    f = c._last_fused
    b, K, nu = f["b"], f["K"], f["nu"]
    c._ensure_block(b)
    costs = torch.from_numpy(np.ascontiguousarray(-np.asarray(rewards), dtype=np.float32)).to(c.device)
    n = costs.numel()
    mode, lam, k, tie = c.optimizer.fused_update_args()
    scratch = torch.zeros(int(L.jh_update_fused_scratch_floats(n, K, nu)), dtype=torch.float32, device=c.device)
    out = torch.zeros(2 * K * nu, dtype=torch.float32, device=c.device)
    st = L.jh_update_fused(costs.data_ptr(), None, _lib.ptr(b.nominal), f["noise_p"], f["ldn"], _lib.ptr(b.sigma), _lib.ptr(b.lohi), n, 0, K, nu, mode, lam, k, tie, 0, None, 0, 0,
                           scratch.data_ptr(), out.data_ptr(), out.data_ptr() + 4 * K * nu, None, 0)
    _lib.check(st, "jh_update_fused")
    torch.cuda.synchronize()
    return out.cpu().numpy()[: K * nu].astype(np.float64).reshape(K, nu)


@pytest.mark.parametrize("task", ["cartpole", "leap_cube"])
def test_identical_members_match_a_plain_controller(gpu, task):
    """Three identical descriptions, the default assignment [0, 1, 2], MPPI: three plan steps in closed sequence from the same seed leave nominal_knots and rewards where
    make_controller's controller leaves them, bit for bit; the traces are those of a plain controller that re-rolls its elites (the launch writes no trace buffer)."""
    from judo_amd.controller import make_controller
    from judo_amd.randomized import RandomizedController, make_randomized_controller

    desc = _task(task).desc
    rn = make_randomized_controller(task, "mppi", [copy.deepcopy(desc) for _ in range(3)])
    assert isinstance(rn, RandomizedController) and rn.num_members == 3 and rn.blocks == 3 and rn.assignment == [0, 1, 2] and len(rn.descriptions) == 3
    plain = make_controller(task, "mppi")
    plain.fused_traces = False
    for c in (rn, plain):
        _configure(c, "mppi")
    for step in range(3):
        for c in (rn, plain):
            _set_state(c, step)
            c.update_action()
        _same(rn.nominal_knots, plain.nominal_knots, f"{task} step {step}: nominal_knots")
        _same(rn.rewards, plain.rewards, f"{task} step {step}: rewards")
        _same(rn.traces, plain.traces, f"{task} step {step}: traces")


@pytest.mark.parametrize("task,opt,pert,a", [("cartpole", "mppi", CARTPOLE, [2, 0, 1]), ("cartpole", "cem", CARTPOLE, [1, 1, 0, 2, 2, 2]), ("cartpole", "ps", CARTPOLE, [2, 0, 1, 0]),
                                             ("leap_cube", "mppi", [LEAP_A, LEAP_B], [2, 0, 1, 0])])
def test_distinct_members_first_plan_step(gpu, task, opt, pert, a):
    """M = 3 distinct descriptions, the first plan step from one seed and state: block g of the rewards is that block of a plain controller on descriptions[a[g]] (so
    the first rollout of a later block carries its noise: it is not that plant's nominal rollout), and nominal_knots is jh_update_fused on those rewards."""
    from judo_amd.randomized import make_randomized_controller

    descs = _descriptions(task, pert)
    rn = make_randomized_controller(task, opt, descs, blocks=len(a))
    rn.assignment = a
    plains = [_plain_on(task, opt, d) for d in descs]
    for c in [rn] + plains:
        _configure(c, opt)
        c.update_action()
    want = _stitch(plains, a)
    _same(rn.rewards, want, f"{task} {opt} {a}: rewards against the plain controllers' blocks")
    nb = N // len(a)
    assert len({p.rewards.tobytes() for p in plains}) == 3
    # the nominal rule: global rollout 0 alone drops its noise.  It shows where the noise shows in the cost: on cartpole; over leap_cube's 8 steps from the home state the
    # cube is in free fall and no rollout's cost sees the hand (tests/test_gpu_plan_randomized.py asserts the rule for the leap kernel from the settled state)
    assert rn.rewards[0] == plains[a[0]].rewards[0]
    noise_shows = plains[a[1]].rewards[nb] != plains[a[1]].rewards[0]
    assert noise_shows or task == "leap_cube"
    if noise_shows:
        assert rn.rewards[nb] != plains[a[1]].rewards[0]
    _same(rn.nominal_knots, _update_fused(rn, want), f"{task} {opt} {a}: nominal_knots against jh_update_fused on the stitched rewards")
    if opt == "mppi":  # (every cost enters the MPPI weights)
        for b, p in enumerate(plains):
            assert (rn.nominal_knots != p.nominal_knots).any(), b
    assert np.isfinite(rn.nominal_knots).all() and rn.traces.shape[0] == TRACES * len(rn.trace_sensors) * (H - 1)
    assert rn.model is rn.model_set.models[0] and rn.model.desc is descs[0]  # member 0 is the nominal plant
    # what belongs to which plant, against numpy on the downloaded rewards
    plant = rn.plant_of_rollout
    assert plant.shape == (N,) and plant.tolist() == [p for p in a for _ in range(nb)]
    got = rn.plant_rewards()
    for m in range(3):
        _same(got[m : m + 1], np.array([rn.rewards[np.repeat(np.asarray(a), nb) == m].mean()]), f"plant_rewards[{m}]")


def test_assignment_weights_and_members_between_plan_steps(gpu):
    """Two controllers in lockstep.  An assignment set between steps is the assignment of the next step; `set_weights` apportions the blocks; a plant without a block
    has a NaN mean; `set_member` replaces a plant."""
    from judo_amd.models import scaled_description
    from judo_amd.randomized import make_randomized_controller

    descs = _descriptions("cartpole", CARTPOLE)
    x, y = make_randomized_controller("cartpole", "mppi", descs), make_randomized_controller("cartpole", "mppi", descs)
    plains = [_plain_on("cartpole", "mppi", d) for d in descs]
    for c in [x, y] + plains:
        _configure(c, "mppi")
        c.update_action()
    _same(x.nominal_knots, y.nominal_knots, "step 0")
    _same(x.rewards, _stitch(plains, [0, 1, 2]), "step 0: the default assignment")
    x.assignment = [1, 2, 0]
    assert x.assignment == [1, 2, 0] and x.plant_of_rollout.tolist() == [0] * 16 + [1] * 16 + [2] * 16  # (still the last step's, until the next one ran)
    for p in plains:  # (the plain controllers follow y's nominal: they stay comparable with y, and with x's rollouts through the shared noise alone)
        p.nominal_knots, p.times = y.nominal_knots.copy(), y.times.copy()
        p.update_spline(p.times, p.nominal_knots)
    x.nominal_knots, x.times = y.nominal_knots.copy(), y.times.copy()
    x.update_spline(x.times, x.nominal_knots)
    for c in [x, y] + plains:
        _set_state(c, 1)
        c.update_action()
    _same(y.rewards, _stitch(plains, [0, 1, 2]), "step 1: y kept its assignment")
    _same(x.rewards, _stitch(plains, [1, 2, 0]), "step 1: x follows the assignment set between the steps")
    assert x.plant_of_rollout.tolist() == [1] * 16 + [2] * 16 + [0] * 16
    assert (x.nominal_knots != y.nominal_knots).any()
    x.set_weights([1, 0, 1], blocks=4)
    assert x.assignment == [0, 0, 2, 2] and x.blocks == 4
    _set_state(x, 2)
    x.update_action()
    pr = x.plant_rewards()
    assert np.isnan(pr[1]) and pr[0] == x.rewards[:24].mean() and pr[2] == x.rewards[24:].mean()
    new = scaled_description(descs[0], body_mass={"pole": 2.0, "cart": 0.8})
    before = x.rewards.copy()
    x.set_member(2, new)
    assert x.descriptions[2] is new and x.model_set.info()["distinct_from_first"] == 2
    x.optimizer.seed(77)
    _set_state(x, 2)
    x.update_action()
    assert x.rewards.shape == before.shape and np.isfinite(x.rewards).all()
    with pytest.raises(ValueError, match="member 3"):
        x.set_member(3, new)


def test_one_library_call_per_iteration(gpu, monkeypatch):
    """update_action() is one jh_plan_step_randomized per optimiser iteration and no other plan-step entry, counted on the bound symbols."""
    from judo_amd import _lib
    from judo_amd.randomized import make_randomized_controller

    L = _lib.lib()
    calls = {"jh_plan_step_randomized": 0, "jh_plan_step_ensemble": 0, "jh_plan_step": 0, "jh_plan_step_batch_models": 0, "jh_update_fused": 0, "jh_rollout_cost_traced": 0}

    def counted(name):
        fn = getattr(L, name)

        def wrapper(*a):
            calls[name] += 1
            return fn(*a)

        return wrapper

    for name in calls:
        monkeypatch.setattr(L, name, counted(name))
    rn = make_randomized_controller("cartpole", "cem", _descriptions("cartpole", CARTPOLE))
    _configure(rn, "cem")
    rn.controller_cfg.max_opt_iters = 2
    rn.update_action()
    assert calls == {"jh_plan_step_randomized": 2, "jh_plan_step_ensemble": 0, "jh_plan_step": 0, "jh_plan_step_batch_models": 0, "jh_update_fused": 0, "jh_rollout_cost_traced": 0}
    rn.optimizer.config.num_rollouts = 2 * N  # a live change of num_rollouts that the blocks divide
    _set_state(rn, 1)
    rn.update_action()
    assert calls["jh_plan_step_randomized"] == 4 and rn.rewards.shape == (2 * N,) and rn.plant_of_rollout.shape == (2 * N,)
    rn.optimizer.config.num_rollouts = 2 * N + 1  # ... and one they do not
    with pytest.raises(ValueError, match=r"num_rollouts % blocks != 0"):
        rn.update_action()
    assert calls["jh_plan_step_randomized"] == 4


def test_refusals(gpu):
    """Every ValueError of the interface, each naming its reason, before anything is launched."""
    from judo_amd.ensemble import make_ensemble_controller
    from judo_amd.ensemble_fleet import EnsembleFleet
    from judo_amd.fleet import ControllerFleet
    from judo_amd.randomized import make_randomized_controller

    descs = _descriptions("cartpole", CARTPOLE)

    def fresh(task="cartpole"):
        c = make_randomized_controller(task, "mppi", descs)
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
        make_randomized_controller("fr3_pick", "cem", [_task("fr3_pick").desc])
    with pytest.raises(ValueError, match="Spot policy"):
        make_randomized_controller("spot_navigate", "mppi", [_task("spot_navigate").desc])
    with pytest.raises(ValueError, match="int section|header|float section"):
        make_randomized_controller("cartpole", "mppi", [descs[0], _task("cylinder_push").desc])
    # the blocks and the assignment
    seven = make_randomized_controller("cartpole", "mppi", descs, blocks=7)
    _configure(seven, "mppi")
    with pytest.raises(ValueError, match=r"num_rollouts % blocks != 0: 48 rollouts do not split into 7"):
        seven.update_action()
    with pytest.raises(ValueError, match="JH_MAX_PLANT_BLOCKS"):
        make_randomized_controller("cartpole", "mppi", descs, blocks=65)
    with pytest.raises(ValueError, match="2 weights for M = 3"):
        make_randomized_controller("cartpole", "mppi", descs, weights=[1, 1])
    with pytest.raises(ValueError, match=r"assignment\[1\] = 3 outside \[0, M = 3\)"):
        c.assignment = [0, 3, 1]
    with pytest.raises(ValueError, match=r"assignment\[0\] = -1"):
        c.assignment = [-1, 0, 1]
    assert c.assignment == [0, 1, 2]  # (a refused assignment changes nothing)
    c.assignment = [0, 1, 2, 0, 1]  # (five blocks are an assignment; that they do not divide 48 rollouts is the plan step's to say)
    with pytest.raises(ValueError, match=r"num_rollouts % blocks != 0"):
        c.update_action()
    c.assignment = [0, 1, 2]
    # the fleets plan every member on one plant, or on all of them: a randomised controller is neither
    with pytest.raises(ValueError, match="fleet member 0 is a RandomizedController.*jh_plan_step_randomized"):
        ControllerFleet([c, fresh()])
    ens = make_ensemble_controller("cartpole", "mppi", descs)
    with pytest.raises(ValueError, match="fleet member 1 is a RandomizedController.*jh_plan_step_randomized"):
        EnsembleFleet([ens, c])
