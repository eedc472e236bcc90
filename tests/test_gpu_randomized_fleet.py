"""RandomizedFleet: B RandomizedControllers whose plan steps run as ONE jh_plan_step_randomized_batch call per iteration, every member bit for bit where a twin
RandomizedController stepped alone from the same seed, states and assignments is: rewards, nominal_knots, action(t), traces, plant_of_rollout, plant_rewards() and
the position of the optimizer's noise stream.  No tolerance anywhere."""

import numpy as np
import pytest

from tests.test_gpu_ensemble_controller import _descriptions
from tests.test_gpu_fleet_models import _count, _set_state
from tests.test_gpu_model_set import CARTPOLE, LEAP_A, LEAP_B

pytestmark = pytest.mark.gpu

TRACES = 3


def _configure(c, i, opt, n_rollouts, h):
    """Member i's configuration: a seed of its own, so members of a fleet differ in their noise as well as in their states."""
    c.optimizer.config.num_rollouts = n_rollouts
    c.controller_cfg.horizon = h * c.task.dt
    c.controller_cfg.max_num_traces = TRACES
    if opt == "cem":
        c.optimizer.sigma = ((c.optimizer.sigma_min + c.optimizer.sigma_max) / 2) * np.ones((c.optimizer.num_nodes, c.nu))
    np.random.seed(100 + i)  # (Task.reset draws the start state from numpy's global stream)
    c.reset()
    assert c.num_timesteps == h
    c.optimizer.seed(1000 + i)


def _noise_position(c):
    """Draws the controller has consumed from its optimizer's noise stream: a controller stepped alone draws the next iteration's noise ahead of time (`prefetch_noise`:
    the same numbers, earlier), which the counter already includes and the plan steps so far have not used."""
    return c.optimizer._generator.draws - (1 if c._noise_ahead is not None else 0)


def _snapshot(c):
    t = c.times[0] + 0.5 * (c.times[-1] - c.times[0])
    return dict(nominal_knots=np.array(c.nominal_knots), rewards=np.array(c.rewards), traces=np.array(c.traces), action=np.array(c.action(t)), plant_of_rollout=np.array(c.plant_of_rollout),
                plant_rewards=np.array(c.plant_rewards()), sigma=np.atleast_1d(np.asarray(getattr(c.optimizer, "sigma", 0.0))).copy(),
                noise_position=np.array([_noise_position(c)], dtype=np.int64))


def _assert_same(got, want, what):
    for key in want:
        x, y = np.ascontiguousarray(got[key]), np.ascontiguousarray(want[key])
        assert x.shape == y.shape and x.dtype == y.dtype, f"{what}: {key}"
        assert x.tobytes() == y.tobytes(), f"{what}: {key} differs"


CASES = [("cartpole", "mppi", 3, 48, 8, CARTPOLE, [[2, 0, 1], [0, 0, 2], [1, 2, 2]], [[0, 1, 2], [2, 2, 1], [1, 0, 0]]),
         ("cartpole", "cem", 3, 48, 8, CARTPOLE, [[2, 0, 1, 1], [0, 0, 2, 1], [1, 2, 2, 0]], [[0, 1, 2, 2], [2, 2, 1, 0], [1, 0, 0, 0]]),
         ("leap_cube", "mppi", 2, 24, 8, [LEAP_A, LEAP_B], [[2, 0, 1, 0], [1, 1, 0, 2]], [[0, 1, 2, 2], [2, 0, 0, 1]])]


@pytest.mark.parametrize("task,opt,B,n_rollouts,h,pert,first,second", CASES)
def test_fleet_equals_lone_randomized_controllers(gpu, monkeypatch, task, opt, B, n_rollouts, h, pert, first, second):
    """Two plan steps with update_states between them, every member with its own seed, state and assignment; between the two, every member's assignment is changed and
    one member's weights are.  Then `set_member` on one member, which switches the launch from the shared set of M to all B * M plants; then a member that leaves the
    fleet goes on alone.  One jh_plan_step_randomized_batch per iteration and no other plan-step entry, counted on the bound symbols."""
    from judo_amd.models import scaled_description
    from judo_amd.randomized import RandomizedController, make_randomized_controller
    from judo_amd.randomized_fleet import RandomizedFleet, make_randomized_fleet

    descs = _descriptions(task, pert)
    M, G = len(descs), len(first[0])
    fleet = make_randomized_fleet(task, opt, B, descs, blocks=G)
    assert isinstance(fleet, RandomizedFleet) and len(fleet) == B and all(isinstance(c, RandomizedController) and c.num_members == M and c.blocks == G for c in fleet)
    assert all(c.assignment == [g % M for g in range(G)] for c in fleet)
    twins = [make_randomized_controller(task, opt, descs, blocks=G) for _ in range(B)]
    for i in range(B):
        _configure(fleet[i], i, opt, n_rollouts, h)
        _configure(twins[i], i, opt, n_rollouts, h)
        fleet[i].assignment = twins[i].assignment = first[i]
    names = ["jh_plan_step_randomized_batch", "jh_plan_step_randomized", "jh_plan_step_ensemble_batch", "jh_plan_step_batch_models", "jh_plan_step_batch", "jh_plan_step"]
    calls = _count(monkeypatch, names)

    def step_and_compare(step, what):
        for i in range(B):  # (member i at plan step `step`: a state and goal of its own)
            _set_state(fleet[i], 10 * step + i)
            _set_state(twins[i], 10 * step + i)
        before = dict(calls)
        fleet.update_action()
        want = {k: 0 for k in names}
        want["jh_plan_step_randomized_batch"] = fleet[0].max_opt_iters
        assert {k: calls[k] - before[k] for k in calls} == want
        for i in range(B):
            twins[i].update_action()
            _assert_same(_snapshot(fleet[i]), _snapshot(twins[i]), f"{task} {opt} member {i} {what}")
            assert fleet[i].rewards.shape == (n_rollouts,)

    step_and_compare(0, "step 0")
    assert [c.plant_of_rollout.tolist() for c in fleet] == [np.repeat(a, n_rollouts // G).tolist() for a in first]
    for i in range(B):
        fleet[i].assignment = twins[i].assignment = second[i]
    w = [1.0, 0.0, 2.0][:M]
    fleet[B - 1].set_weights(w)
    twins[B - 1].set_weights(w)
    assert fleet[B - 1].assignment != second[B - 1] and 1 not in fleet[B - 1].assignment
    step_and_compare(1, "step 1, after new assignments and weights")
    assert fleet._model_set.info()["B"] == M  # every member's plants are member 0's, list for list: the shared set
    assert np.isnan(fleet[B - 1].plant_rewards()[1])  # (a plant without a block)
    r = [np.asarray(c.rewards) for c in fleet]
    assert all((r[a] != r[b]).any() for a in range(B) for b in range(a + 1, B))  # the members plan different problems

    # a plant replaced on one member: the launch goes from the shared set to B * M, and the member's next step still equals the lone controller's
    new = scaled_description(descs[1], body_mass={"pole": 2.0} if task == "cartpole" else {"cube": 1.25})
    old_set = fleet._model_set
    fleet[0].set_member(1, new)
    twins[0].set_member(1, new)
    fleet[0].assignment = twins[0].assignment = [1] * G
    step_and_compare(2, "after set_member")
    assert fleet._model_set is not old_set and fleet._model_set.info()["B"] == B * M

    # a member taken out of the fleet goes on alone, bit for bit
    out, ref = fleet[B - 1], twins[B - 1]
    _set_state(out, 77)
    _set_state(ref, 77)
    before = dict(calls)
    out.update_action()
    assert calls["jh_plan_step_randomized_batch"] == before["jh_plan_step_randomized_batch"] and calls["jh_plan_step_randomized"] == before["jh_plan_step_randomized"] + out.max_opt_iters
    ref.update_action()
    _assert_same(_snapshot(out), _snapshot(ref), f"{task} member {B - 1} on its own")


def test_admission_and_refusals(gpu):
    """Every ValueError of the interface, each naming its reason, before anything is launched."""
    from judo_amd import _lib
    from judo_amd.ensemble import make_ensemble_controller
    from judo_amd.ensemble_fleet import EnsembleFleet
    from judo_amd.fleet import ControllerFleet, make_controller_fleet
    from judo_amd.randomized import make_randomized_controller
    from judo_amd.randomized_fleet import RandomizedFleet, make_randomized_fleet

    descs = _descriptions("cartpole", CARTPOLE)

    def member(ds=descs, n=48, blocks=None):
        c = make_randomized_controller("cartpole", "mppi", ds, blocks=blocks)
        _configure(c, 0, "mppi", n, 8)
        return c

    RandomizedFleet([member(), member()])
    with pytest.raises(ValueError, match=r"member 1 .*number of plants M: 2 against 3"):
        RandomizedFleet([member(), member(descs[:2])])
    with pytest.raises(ValueError, match=r"member 1 .*number of blocks G: 6 against 3"):
        RandomizedFleet([member(), member(blocks=6)])
    with pytest.raises(ValueError, match=r"member 1 .*num_rollouts"):
        RandomizedFleet([member(), member(n=24)])
    kept = member()
    kept.keep_candidates = True
    with pytest.raises(ValueError, match=r"member 1 does not run its iteration as one jh_plan_step_randomized call \(keep_candidates"):
        RandomizedFleet([member(), kept])
    running = member()
    running.controller_cfg.action_normalizer = "running"
    with pytest.raises(ValueError, match=r"member 0 .*running normaliser"):
        RandomizedFleet([running, member()])
    with pytest.raises(ValueError, match="not a RandomizedController"):
        RandomizedFleet([member(), make_controller_fleet("cartpole", "mppi", 1)[0]])
    with pytest.raises(ValueError, match="not a RandomizedController"):
        RandomizedFleet([member(), make_ensemble_controller("cartpole", "mppi", descs)])
    # the blocks: their number is a member's live setting, whether they divide num_rollouts is the plan step's to say -- and a member that changes G alone splits the fleet
    seven = RandomizedFleet([member(blocks=7), member(blocks=7)])
    with pytest.raises(ValueError, match=r"num_rollouts % blocks != 0: 48 rollouts do not split into 7"):
        seven.update_action()
    fleet = RandomizedFleet([member(), member()])
    fleet[1].assignment = [0, 1, 2, 0]
    with pytest.raises(ValueError, match=r"member 1 .*number of blocks G: 4 against 3"):
        fleet.update_action()
    fleet[1].assignment = [0, 1, 2]
    fleet.update_action()
    assert all(np.isfinite(c.nominal_knots).all() for c in fleet)
    # B * G above the bytes of the table in the kernel arguments, from the shim's constant; refused before a controller is made
    limit = _lib.MAX_FLEET_PLANT_BLOCKS
    B_over = limit // 64 + 1
    with pytest.raises(ValueError, match=rf"B \* G = {B_over} \* 64 = {B_over * 64} .*JH_MAX_FLEET_PLANT_BLOCKS"):
        make_randomized_fleet("cartpole", "mppi", B_over, descs, blocks=64)
    with pytest.raises(ValueError, match="JH_MAX_PLANT_BLOCKS"):
        make_randomized_fleet("cartpole", "mppi", 2, descs, blocks=65)
    with pytest.raises(ValueError, match="number of plants M"):
        make_randomized_fleet("cartpole", "mppi", 2, [descs, descs[:2]])
    with pytest.raises(ValueError, match="2 weights for M = 3"):
        make_randomized_fleet("cartpole", "mppi", 2, descs, weights=[1, 1])
    # the other fleets still refuse a randomised member, and now say where it goes
    with pytest.raises(ValueError, match=r"fleet member 0 is a RandomizedController.*jh_plan_step_randomized.*RandomizedFleet"):
        ControllerFleet([member(), member()])
    with pytest.raises(ValueError, match=r"fleet member 1 is a RandomizedController.*jh_plan_step_randomized.*RandomizedFleet"):
        EnsembleFleet([make_ensemble_controller("cartpole", "mppi", descs), member()])
