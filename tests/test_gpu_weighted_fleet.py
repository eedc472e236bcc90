"""WeightedEnsembleFleet and FR3WeightedEnsembleFleet: B ensemble controllers, each under its own risk measure -- `worst`, general plant weights, one-hot weights --
whose plan steps run as ONE jh_plan_step_ensemble_batch[_phases]_risk call per iteration, every member bit for bit where a twin controller stepped alone from the same
seed and states is.  Between the plan steps a member gets new weights and another returns to `worst` through `set_weights(None)`, without leaving the fleet.  Then the
loop the fleet was made for: two estimators whose truths are different plants hand their posteriors to the members of one fleet (`apply_risk`), and the fleet's next
costs are the restatement with those weights.  No tolerance anywhere."""

import numpy as np
import pytest

from tests.test_gpu_ensemble_controller import _descriptions
from tests.test_gpu_ensemble_fleet import _assert_same, _configure, _snapshot, _states
from tests.test_gpu_fleet_models import _count
from tests.test_gpu_model_set import CARTPOLE, LEAP_A, LEAP_B

pytestmark = pytest.mark.gpu

WORST = [1, 2, 3]
WEIGHTS = [None, [0.2, 0.5, 0.3], [0.0, 0.0, 1.0]]  # member 0 under `worst` = 1, member 1 general weights, member 2 one-hot
TAILS = [None, 0.4, 1.0]


def _risk(c, weights, tail):
    if weights is not None:
        c.set_weights(weights, tail)


@pytest.mark.parametrize("task,n_rollouts,h", [("cartpole", 64, 8), ("leap_cube", 64, 4)])
def test_fleet_of_three_equals_twin_controllers(gpu, monkeypatch, task, n_rollouts, h):
    from judo_amd.ensemble import EnsembleController, aggregate_costs_host, aggregate_costs_weighted_host, make_ensemble_controller
    from judo_amd.ensemble_fleet import EnsembleFleet
    from judo_amd.weighted_fleet import WeightedEnsembleFleet, make_weighted_ensemble_fleet

    descs = _descriptions(task, CARTPOLE if task == "cartpole" else [LEAP_A, LEAP_B])  # M = 3, shared by every member
    fleet = make_weighted_ensemble_fleet(task, "mppi", 3, descs, worst=WORST, weights=[w or [1, 1, 1] for w in WEIGHTS], tail=[t or 1.0 for t in TAILS])
    fleet[0].set_weights(None)  # (the maker gives every member weights or none: member 0 goes back to `worst`)
    assert isinstance(fleet, WeightedEnsembleFleet) and isinstance(fleet, EnsembleFleet) and all(type(c) is EnsembleController for c in fleet)
    assert [c.worst for c in fleet] == WORST and fleet[0].weights is None and fleet[2].weights.tolist() == [0.0, 0.0, 1.0] and fleet[1].tail == float(np.float32(0.4))
    twins = [make_ensemble_controller(task, "mppi", descs, worst=WORST[i]) for i in range(3)]
    for i in range(3):
        _risk(twins[i], WEIGHTS[i], TAILS[i])
        _configure(fleet[i], i, n_rollouts, h)
        _configure(twins[i], i, n_rollouts, h)
    names = ["jh_plan_step_ensemble_batch_risk", "jh_plan_step_ensemble_batch", "jh_plan_step_ensemble", "jh_plan_step_ensemble_weighted"]
    calls = _count(monkeypatch, names)

    def step_and_compare(step, what):
        _states(fleet, twins, step)
        before = dict(calls)
        fleet.update_action()
        assert {k: calls[k] - before[k] for k in calls} == {**{k: 0 for k in names}, "jh_plan_step_ensemble_batch_risk": fleet[0].max_opt_iters}  # one launch chain for all three
        for i in range(3):
            twins[i].update_action()
            _assert_same(_snapshot(fleet[i]), _snapshot(twins[i]), f"{task} member {i} {what}")
            mc, c = fleet[i].member_costs, fleet[i]
            want = aggregate_costs_host(mc, c.worst) if c.weights is None else aggregate_costs_weighted_host(mc, c.weights, c.tail)
            assert c.costs_device.cpu().numpy().tobytes() == want.tobytes(), f"{task} member {i} {what}: costs against the restatement"

    step_and_compare(0, "step 0")
    assert np.asarray(fleet[2].rewards, np.float64).tobytes() == fleet[2].member_rewards[2].tobytes()  # one-hot, tail 1: plant 2's rewards
    # new weights for one member, another back to `worst`: both without leaving the fleet, both at the next plan step
    for cs in (fleet, twins):
        cs[1].set_weights([3.0, 1.0, 0.0], 0.25)
        cs[2].set_weights(None)
        cs[0].worst = 2
    step_and_compare(1, "after set_weights and set_weights(None)")
    assert fleet[2].weights is None and fleet[2].worst == 3
    with pytest.raises(ValueError, match=r"fleet member 1 has plant weights set.*one `worst` per controller"):  # the unweighted fleet still refuses the same members
        EnsembleFleet(list(fleet))


def test_fr3_fleet_in_different_phases_equals_twin_controllers(gpu):
    from judo_amd.fr3_ensemble import FR3EnsembleController, FR3EnsembleFleet, make_fr3_ensemble_controller
    from judo_amd.weighted_fleet import FR3WeightedEnsembleFleet, make_fr3_weighted_ensemble_fleet
    from tests.test_fr3_plants_host import plants
    from tests.test_gpu_fr3_axis_controllers import LIFTED, N, _snap_ens
    from tests.test_gpu_fr3_fleet import _assert_same as same
    from tests.test_gpu_fr3_fleet import _configure as configure
    from tests.test_gpu_fr3_fleet import _set_state as set_state

    descs = list(plants()[:3])
    fleet = make_fr3_weighted_ensemble_fleet("cem", 3, descs, worst=WORST)
    assert isinstance(fleet, FR3WeightedEnsembleFleet) and all(type(c) is FR3EnsembleController for c in fleet)
    twins = [make_fr3_ensemble_controller("cem", descs, worst=WORST[i]) for i in range(3)]
    for i in range(3):
        for c in (fleet[i], twins[i]):
            _risk(c, WEIGHTS[i], TAILS[i])
            configure(c, i, n=N)
    for step in range(2):
        if step == 1:
            for cs in (fleet, twins):
                cs[1].set_weights([3.0, 1.0, 0.0], 0.25)
                cs[2].set_weights(None)
        for i in range(3):
            cube = LIFTED if (i == 0 and step >= 1) else None
            set_state(fleet[i], i, step, cube)
            set_state(twins[i], i, step, cube)
        fleet.update_action()
        for i in range(3):
            twins[i].update_action()
            same(_snap_ens(fleet[i]), _snap_ens(twins[i]), f"member {i} step {step}")
        assert [c.task.phase for c in fleet] == ([0, 1, 2] if step == 0 else [1, 1, 2])  # the members in different phases, member 0's changing
    with pytest.raises(ValueError, match=r"fleet member 1 has plant weights set"):
        FR3EnsembleFleet(list(fleet))


def test_two_estimators_one_fleet_launch(gpu, monkeypatch):
    """B = 2 on cartpole.  Robot i's truth is plant i + 1: its estimator finds it from 2 * horizon observed steps, `apply_risk(fleet[i], floor=0.1)` sets the weights of
    the formula on the member, and the fleet's next plan step -- one call -- has, per member, the costs of the restatement with those weights."""
    import torch

    from judo_amd.ensemble import aggregate_costs_weighted_host
    from judo_amd.identify import PlantEstimator
    from judo_amd.weighted_fleet import make_weighted_ensemble_fleet
    from tests import test_gpu_materialize_plants as closed
    from tests.test_gpu_plant_estimator import W, _cartpole_descriptions, _reference
    from tests.test_gpu_plant_estimator import _configure as configure

    ref = _reference("cartpole")
    H = ref["H"]
    fleet = make_weighted_ensemble_fleet("cartpole", "mppi", 2, _cartpole_descriptions(), worst=1)
    for c in fleet:
        configure(c)
    fleet.update_action()  # (both members under `worst`: every tail word 0.0)
    ests = [PlantEstimator.for_controller(c, horizon=H, windows=W, state_sigma=1e-4) for c in fleet]
    for i, est in enumerate(ests):
        truth = ref["models"][i + 1]
        x = torch.from_numpy(closed._x0("cartpole", 1, 9 + i)[0]).to(gpu)
        us = torch.from_numpy(closed._controls("cartpole", 1, 2 * H, 10 + i)).to(gpu)
        for t in range(2 * H):
            u = us[:, t : t + 1].contiguous()
            x_next = closed._single(truth, x, 0, u, want_sensors=False)[0][0, 0].clone()
            est.observe_step(x, u[0, 0], x_next)
            x = x_next
        w = est.apply_risk(fleet[i], floor=0.1)
        assert est.map == i + 1 and est.posterior[i + 1] > 0.99, (i, est.posterior, est.errors)
        formula = 0.9 * est.posterior + 0.1 / 3
        assert np.array_equal(w, formula) and np.array_equal(fleet[i].weights, (formula / formula.sum()).astype(np.float32))
    assert not np.array_equal(fleet[0].weights, fleet[1].weights)
    calls = _count(monkeypatch, ["jh_plan_step_ensemble_batch_risk", "jh_plan_step_ensemble_weighted"])
    fleet.update_action()
    torch.cuda.synchronize()
    assert calls == {"jh_plan_step_ensemble_batch_risk": 1, "jh_plan_step_ensemble_weighted": 0}
    for i, c in enumerate(fleet):
        mc = c.member_costs
        want = aggregate_costs_weighted_host(mc, c.weights, c.tail)
        assert c.costs_device.cpu().numpy().tobytes() == want.tobytes(), f"member {i}: costs after apply_risk"
        assert np.asarray(c.rewards, np.float64).tobytes() == (-want.astype(np.float64)).tobytes(), f"member {i}: rewards after apply_risk"
        assert (want != mc.max(axis=0)).any() and np.isfinite(c.nominal_knots).all()  # no longer the worst case over all three plants
