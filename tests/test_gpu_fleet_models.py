"""ControllerFleet with a model description per member (randomised physics): the members keep their own GpuModel, the fleet plans them in one
jh_plan_step_batch_models call per iteration, and every member is bit for bit where a controller alone on the same description would be."""

import copy

import numpy as np
import pytest

from tests.test_gpu_fleet import _assert_same, _snapshot
from tests.test_gpu_model_set import CARTPOLE, LEAP_A, LEAP_B, _settled

pytestmark = pytest.mark.gpu

H, TRACES = 8, 3


def _descriptions(task, perturbations):
    from judo_amd.models import scaled_description
    from judo_amd.tasks import get_registered_tasks

    desc = get_registered_tasks()[task][0]().desc
    return [copy.deepcopy(desc)] + [scaled_description(desc, **kw) for kw in perturbations]


def _alone(task, opt, desc):
    """A controller on its own built on `desc` (a fleet of one is never planned as a fleet here: only its member's own update_action() runs)."""
    from judo_amd.fleet import make_controller_fleet

    return make_controller_fleet(task, opt, 1, descriptions=[desc])[0]


def _configure(c, i, n_rollouts):
    """tests/test_gpu_fleet.py's member configuration with the rollout count as an argument; every member gets the SAME seed, so members differ through their plants."""
    c.optimizer.config.num_rollouts = n_rollouts
    c.controller_cfg.horizon = H * c.task.dt
    c.controller_cfg.max_num_traces = TRACES
    np.random.seed(100)  # (Task.reset draws the start state from numpy's global stream)
    c.reset()
    assert c.num_timesteps == H
    c.optimizer.seed(1000)


def _set_state(c, step):
    """The same plant state, time and goal for every member at plan step `step`."""
    rng = np.random.default_rng(step)
    if c.task.name == "leap_cube":
        x = _settled("leap_cube", 60).copy()  # (the cube rests in the hand: its mass and friction matter from the first step on)
        x[7:23] += 0.01 * rng.standard_normal(16)
        q = rng.standard_normal(4)
        meta = {"goal_quat": q / np.linalg.norm(q)}
    else:
        x = np.array([0.1, 0.3, 0.0, 0.0]) + 0.02 * rng.standard_normal(4)
        meta = {}
    c.update_states(x[: c.task.nq], x[c.task.nq :], 0.03 * step, meta)


def _count(monkeypatch, names):
    from judo_amd import _lib

    L = _lib.lib()
    calls = {n: 0 for n in names}

    def counted(name):
        fn = getattr(L, name)

        def wrapper(*a):
            calls[name] += 1
            return fn(*a)

        return wrapper

    for name in names:
        monkeypatch.setattr(L, name, counted(name))
    return calls


@pytest.mark.parametrize("task,opt,n_rollouts,steps,perturbations", [("cartpole", "mppi", 8, 3, CARTPOLE), ("leap_cube", "mppi", 32, 1, [LEAP_A, LEAP_B])])
def test_fleet_with_a_description_per_member_equals_standalone_controllers(gpu, monkeypatch, task, opt, n_rollouts, steps, perturbations):
    from judo_amd.fleet import make_controller_fleet

    descs = _descriptions(task, perturbations)
    B = len(descs)
    fleet = make_controller_fleet(task, opt, B, descriptions=descs)
    assert all(fleet[i].model is not fleet[0].model for i in range(1, B)), "members with distinct descriptions share one GpuModel"
    assert all(fleet[i].task.desc is descs[i] and fleet[i].model.desc is descs[i] for i in range(B))
    alone = [_alone(task, opt, d) for d in descs]
    for i in range(B):
        _configure(fleet[i], i, n_rollouts)
        _configure(alone[i], i, n_rollouts)
    calls = _count(monkeypatch, ["jh_plan_step_batch_models", "jh_plan_step_batch", "jh_plan_step"])
    for step in range(steps):
        for i in range(B):
            _set_state(fleet[i], step)
            _set_state(alone[i], step)
        before = dict(calls)
        fleet.update_action()
        iters = fleet[0].max_opt_iters
        assert {k: calls[k] - before[k] for k in calls} == {"jh_plan_step_batch_models": iters, "jh_plan_step_batch": 0, "jh_plan_step": 0}
        for i in range(B):
            alone[i].update_action()
            _assert_same(_snapshot(fleet[i]), _snapshot(alone[i]), f"{task} {opt} member {i} step {step}")
        # same seed, state and goal: the members' rewards differ through their model images alone, in every rollout
        r = [np.asarray(c.rewards) for c in fleet]
        assert all((r[a] != r[b]).all() for a in range(B) for b in range(a + 1, B))
    assert fleet._model_set is not None and fleet._model_set.info()["distinct_from_first"] == B - 1
    # a member taken out of the fleet goes on alone, bit for bit
    out, ref = fleet[B - 1], alone[B - 1]
    _set_state(out, steps)
    _set_state(ref, steps)
    before = dict(calls)
    out.update_action()
    assert calls["jh_plan_step_batch_models"] == before["jh_plan_step_batch_models"] and calls["jh_plan_step"] > before["jh_plan_step"]
    ref.update_action()
    _assert_same(_snapshot(out), _snapshot(ref), f"{task} member {B - 1} on its own")


def test_fleet_of_identical_descriptions_shares_one_model_and_the_old_call(gpu, monkeypatch):
    """Byte-identical images, given as descriptions or not: one GpuModel, jh_plan_step_batch, no model set."""
    from judo_amd.fleet import make_controller_fleet

    desc = _descriptions("cartpole", [])[0]
    fleet = make_controller_fleet("cartpole", "mppi", 3, descriptions=[desc, copy.deepcopy(desc), copy.deepcopy(desc)])
    assert all(c.model is fleet.model for c in fleet)
    for i, c in enumerate(fleet):
        _configure(c, i, 8)
        _set_state(c, 0)
    calls = _count(monkeypatch, ["jh_plan_step_batch_models", "jh_plan_step_batch"])
    fleet.update_action()
    assert calls == {"jh_plan_step_batch_models": 0, "jh_plan_step_batch": fleet[0].max_opt_iters} and fleet._model_set is None


def test_fleet_description_refusals(gpu):
    from judo_amd.fleet import make_controller_fleet

    leap = _descriptions("leap_cube", [LEAP_A])
    edited = copy.deepcopy(leap[0])  # a structural difference: another <exclude> pair moves the pair lists of the int section and nothing else
    edited["excludes"][0] = [6, 10]
    with pytest.raises(ValueError, match="another model image or kernel build.*int section"):
        make_controller_fleet("leap_cube", "mppi", 2, descriptions=[leap[0], edited])
    edited["excludes"] = leap[0]["excludes"][1:]  # one pair less: the int section grows, and the header says so
    with pytest.raises(ValueError, match="another model image or kernel build.*header"):
        make_controller_fleet("leap_cube", "mppi", 2, descriptions=[leap[0], edited])
    with pytest.raises(ValueError, match="2 descriptions for a fleet of 3"):
        make_controller_fleet("leap_cube", "mppi", 3, descriptions=leap)
    fr3 = _descriptions("fr3_pick", [dict(actuator_kp={None: 1.1})])
    with pytest.raises(ValueError, match="fr3_pick"):
        make_controller_fleet("fr3_pick", "mppi", 2, descriptions=fr3)
    with pytest.raises(ValueError, match="fr3_pick"):
        make_controller_fleet("fr3_pick", "mppi", 2)
    spot = _descriptions("spot_base", []) * 2
    with pytest.raises(ValueError, match="Spot fleet"):
        make_controller_fleet("spot_base", "mppi", 2, descriptions=spot)
    # a fleet that mixes kernel builds stays refused, whatever the images
    fleet = make_controller_fleet("leap_cube", "mppi", 2, descriptions=leap)
    fleet[1].model.set_contact_capacity(64)
    with pytest.raises(ValueError, match="kernel build"):
        fleet.update_action()
