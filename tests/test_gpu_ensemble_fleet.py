"""EnsembleFleet: B EnsembleControllers whose plan steps run as ONE jh_plan_step_ensemble_batch call per iteration, every member bit for bit where a twin
EnsembleController stepped alone from the same seed and states is: nominal_knots, rewards, member_costs, traces, action(t)."""

import numpy as np
import pytest

from tests.test_gpu_ensemble_controller import _descriptions
from tests.test_gpu_fleet_models import _count, _set_state
from tests.test_gpu_model_set import CARTPOLE, LEAP_A, LEAP_B

pytestmark = pytest.mark.gpu

H, TRACES = 8, 3


def _configure(c, i, n_rollouts, h=H):
    """Member i's configuration: a seed of its own, so members of a fleet differ in their noise as well as in their states."""
    c.optimizer.config.num_rollouts = n_rollouts
    c.controller_cfg.horizon = h * c.task.dt
    c.controller_cfg.max_num_traces = TRACES
    np.random.seed(100 + i)  # (Task.reset draws the start state from numpy's global stream)
    c.reset()
    assert c.num_timesteps == h
    c.optimizer.seed(1000 + i)


def _snapshot(c):
    t = c.times[0] + 0.5 * (c.times[-1] - c.times[0])
    return dict(nominal_knots=np.array(c.nominal_knots), rewards=np.array(c.rewards), member_costs=np.array(c.member_costs), traces=np.array(c.traces), action=np.array(c.action(t)))


def _assert_same(got, want, what):
    for key in want:
        x, y = np.ascontiguousarray(got[key]), np.ascontiguousarray(want[key])
        assert x.shape == y.shape and x.dtype == y.dtype, f"{what}: {key}"
        assert x.tobytes() == y.tobytes(), f"{what}: {key} differs (max |d| = {np.abs(x - y).max():.3e})"


def _states(fleet, twins, step):
    for i, (c, t) in enumerate(zip(fleet, twins)):  # (member i at plan step `step`: a state and goal of its own)
        _set_state(c, 10 * step + i)
        _set_state(t, 10 * step + i)


@pytest.mark.parametrize("task,opt,B,n_rollouts,h,worst,form", [("cartpole", "mppi", 3, 64, 8, [1, 2, 3], "shared"), ("leap_cube", "mppi", 2, 8, 4, [1, 2], "per_member")])
def test_fleet_equals_twin_ensemble_controllers(gpu, monkeypatch, task, opt, B, n_rollouts, h, worst, form):
    """Three plan steps with update_states between them; then `worst` changed on one member and a plant replaced on another, which take effect at the next plan step; then a
    member that leaves the fleet goes on alone.  One jh_plan_step_ensemble_batch per iteration and no jh_plan_step_ensemble, counted on the bound symbols."""
    from judo_amd.ensemble import EnsembleController, make_ensemble_controller
    from judo_amd.ensemble_fleet import EnsembleFleet, make_ensemble_fleet
    from judo_amd.models import scaled_description

    if task == "cartpole":
        descs = _descriptions(task, CARTPOLE)  # M = 3, shared by every member
        lists = [descs] * B
        fleet = make_ensemble_fleet(task, opt, B, descs, worst=worst)
    else:
        lists = [_descriptions(task, [LEAP_A]), _descriptions(task, [LEAP_B])]  # M = 2, a member's own plants
        fleet = make_ensemble_fleet(task, opt, B, lists, worst=worst)
    M = len(lists[0])
    assert isinstance(fleet, EnsembleFleet) and len(fleet) == B and all(isinstance(c, EnsembleController) and c.num_members == M for c in fleet)
    assert [c.worst for c in fleet] == worst
    twins = [make_ensemble_controller(task, opt, lists[i], worst=worst[i]) for i in range(B)]
    for i in range(B):
        _configure(fleet[i], i, n_rollouts, h)
        _configure(twins[i], i, n_rollouts, h)
    calls = _count(monkeypatch, ["jh_plan_step_ensemble_batch", "jh_plan_step_ensemble", "jh_plan_step_batch_models", "jh_plan_step_batch", "jh_plan_step"])

    def step_and_compare(step, what):
        _states(fleet, twins, step)
        before = dict(calls)
        fleet.update_action()
        assert {k: calls[k] - before[k] for k in calls} == {"jh_plan_step_ensemble_batch": fleet[0].max_opt_iters, "jh_plan_step_ensemble": 0, "jh_plan_step_batch_models": 0,
                                                             "jh_plan_step_batch": 0, "jh_plan_step": 0}
        for i in range(B):
            twins[i].update_action()
            _assert_same(_snapshot(fleet[i]), _snapshot(twins[i]), f"{task} {opt} member {i} {what}")
            assert fleet[i].member_costs.shape == (M, n_rollouts)

    for step in range(3):
        step_and_compare(step, f"step {step}")
    assert fleet._model_set.info()["B"] == (M if form == "shared" else B * M)
    # the members plan different problems: their rewards differ
    r = [np.asarray(c.rewards) for c in fleet]
    assert all((r[a] != r[b]).any() for a in range(B) for b in range(a + 1, B))

    # `worst` on one member, a plant on another: both take effect at the next plan step
    fleet[0].worst = twins[0].worst = M
    new = scaled_description(lists[B - 1][0], body_mass={"pole": 2.0} if task == "cartpole" else {"cube": 1.25})
    old_set = fleet._model_set
    fleet[B - 1].set_member(1, new)
    twins[B - 1].set_member(1, new)
    step_and_compare(3, "after worst and set_member")
    assert fleet._model_set is not old_set and fleet._model_set.info()["B"] == B * M  # (the members' plants are no longer the same list for list)

    # a member taken out of the fleet goes on alone, bit for bit
    out, ref = fleet[B - 1], twins[B - 1]
    _set_state(out, 77)
    _set_state(ref, 77)
    before = dict(calls)
    out.update_action()
    assert calls["jh_plan_step_ensemble_batch"] == before["jh_plan_step_ensemble_batch"] and calls["jh_plan_step_ensemble"] == before["jh_plan_step_ensemble"] + out.max_opt_iters
    ref.update_action()
    _assert_same(_snapshot(out), _snapshot(ref), f"{task} member {B - 1} on its own")


def test_admission(gpu):
    from judo_amd.ensemble import make_ensemble_controller
    from judo_amd.ensemble_fleet import EnsembleFleet, make_ensemble_fleet
    from judo_amd.fleet import ControllerFleet, make_controller_fleet

    descs = _descriptions("cartpole", CARTPOLE)

    def member(ds, n=16):
        c = make_ensemble_controller("cartpole", "mppi", ds)
        _configure(c, 0, n)
        return c

    EnsembleFleet([member(descs), member(descs)])
    with pytest.raises(ValueError, match=r"member 1 .*number of plants M: 2 against 3"):
        EnsembleFleet([member(descs), member(descs[:2])])
    with pytest.raises(ValueError, match=r"member 1 .*num_rollouts"):
        EnsembleFleet([member(descs), member(descs, n=24)])
    kept = member(descs)
    kept.keep_candidates = True
    with pytest.raises(ValueError, match=r"member 1 .*keep_candidates"):
        EnsembleFleet([member(descs), kept])
    with pytest.raises(ValueError, match="not an EnsembleController"):
        EnsembleFleet([member(descs), make_controller_fleet("cartpole", "mppi", 1)[0]])
    with pytest.raises(ValueError, match="number of plants M"):
        make_ensemble_fleet("cartpole", "mppi", 2, [descs, descs[:2]])
    with pytest.raises(ValueError, match="worst = 4"):
        make_ensemble_fleet("cartpole", "mppi", 2, descs, worst=[1, 4])
    # a fleet of plain controllers would plan an ensemble member on its plant 0 alone: refused, with the fleet that does plan it named
    with pytest.raises(ValueError, match=r"member 0 is an EnsembleController.*EnsembleFleet"):
        ControllerFleet([member(descs), member(descs)])
    with pytest.raises(ValueError, match=r"member 1 is an EnsembleController.*EnsembleFleet"):
        ControllerFleet([make_controller_fleet("cartpole", "mppi", 1)[0], member(descs)])
