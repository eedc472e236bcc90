"""The fr3 launch's controller axis through the public classes: an FR3EnsembleController (one arm against M plants), an FR3EnsembleFleet and an FR3RandomizedFleet (B such
arms in one launch) leave every controller bit for bit where the forms the tree already had leave it.  48 rollouts, H = 8, two plan steps with a cube moved between them
so that a phase changes.  No tolerance anywhere.  The plants are D0..D3 of tests/test_fr3_plants_host.py."""

import copy

import numpy as np
import pytest

from tests.test_fr3_plants_host import plants
from tests.test_gpu_fr3_fleet import _assert_same, _configure, _set_state
from tests.test_gpu_fr3_plants import _lone_on, _snap

pytestmark = pytest.mark.gpu

N = 48
LIFTED = [0.7, 0.0, 0.05]


def _snap_ens(c):
    s = _snap(c)
    s["member_costs"] = c.member_costs.copy()
    return s


# ------------------------------------------------------------------------------------------------ 1. the ensemble controller
def test_ensemble_controller_on_identical_plants_is_a_plain_controller(gpu):
    """Three copies of D0, `worst` = 1: the maximum of three equal costs is that cost, so two plan steps in closed sequence, the phase changing between them, leave
    nominal, sigma, rewards, traces and the phase where a plain controller that re-rolls its trace elites leaves them."""
    from judo_amd.controller import make_controller_for
    from judo_amd.ensemble import EnsembleController
    from judo_amd.fr3_ensemble import FR3EnsembleController, make_fr3_ensemble_controller
    from judo_amd.tasks import FR3Pick

    d0 = plants()[0]
    en = make_fr3_ensemble_controller("mppi", [copy.deepcopy(d0) for _ in range(3)], worst=1)
    assert isinstance(en, FR3EnsembleController) and isinstance(en, EnsembleController) and en.num_members == 3 and en.model_set.fr3
    plain = make_controller_for(FR3Pick(), "mppi")
    plain.fused_traces = False
    for c in (en, plain):
        _configure(c, 7, n=N)
    for step in range(2):
        for c in (en, plain):
            _set_state(c, 0, step, LIFTED if step else None)
            c.update_action()
        _assert_same(_snap(en), _snap(plain), f"identical plants step {step}")
        assert en.task.phase == step  # LIFT, then MOVE
        mc = en.member_costs
        assert mc.shape == (3, N) and mc[0].tobytes() == mc[1].tobytes() == mc[2].tobytes()


def test_worst_case_rewards_are_the_row_wise_minimum(gpu):
    """D0..D2 and `worst` = 1: the rewards are the minimum over the members' rewards, rollout by rollout; the members' rows are those of lone controllers on the plants
    with the same noise; `worst` set between the steps takes effect at the next."""
    from judo_amd.ensemble import aggregate_costs_host
    from judo_amd.fr3_ensemble import make_fr3_ensemble_controller

    descs = list(plants()[:3])
    en = make_fr3_ensemble_controller("mppi", descs, worst=1)
    lone = [_lone_on(d, "mppi") for d in descs]
    cs = [en] + lone
    for c in cs:
        _configure(c, 5, n=N)
    noise = np.random.default_rng(3).standard_normal((N - 1, en.optimizer.num_nodes, en.nu)).astype(np.float32)
    for c in cs:
        c.optimizer.injected_noise = noise
        _set_state(c, 2, 0)  # the cube above the goal: PLACE
        c.update_action()
    assert en.task.phase == 2
    mr = en.member_rewards
    assert mr.shape == (3, N) and len({mr[m].tobytes() for m in range(3)}) == 3  # the plants matter
    for m in range(3):
        _assert_same(dict(r=mr[m].astype(np.float32)), dict(r=np.asarray(lone[m].rewards, dtype=np.float32)), f"member {m} against a lone controller on its plant")
    _assert_same(dict(r=np.asarray(en.rewards, dtype=np.float64)), dict(r=mr.min(axis=0)), "worst = 1")
    en.worst = 3
    _set_state(en, 1, 1)  # the cube lifted: MOVE
    en.update_action()
    assert en.task.phase == 1
    want = -aggregate_costs_host(en.member_costs, 3).astype(np.float64)
    _assert_same(dict(r=np.asarray(en.rewards, dtype=np.float64)), dict(r=want), "worst = 3")


# ------------------------------------------------------------------------------------------------ 2. the ensemble fleet
@pytest.mark.parametrize("per_member", [False, True])
def test_ensemble_fleet_equals_lone_ensemble_controllers(gpu, per_member):
    """make_fr3_ensemble_fleet("cem", 3, ...) with worst (1, 2, 1): the members in the phases LIFT, MOVE, PLACE, member 0's cube lifted between the two plan steps (LIFT ->
    MOVE).  Shared plants [D0, D1]; or a member's own ([D0, D1], [D1, D2], [D2, D3]), which the launch reads as one set of six."""
    from judo_amd.fr3_ensemble import FR3EnsembleController, FR3EnsembleFleet, make_fr3_ensemble_controller, make_fr3_ensemble_fleet

    d = plants()
    lists = [[d[i], d[i + 1]] for i in range(3)] if per_member else [[d[0], d[1]]] * 3
    worst = [1, 2, 1]
    fleet = make_fr3_ensemble_fleet("cem", 3, lists if per_member else lists[0], worst=worst)
    assert isinstance(fleet, FR3EnsembleFleet) and len(fleet) == 3 and all(type(c) is FR3EnsembleController for c in fleet) and [c.worst for c in fleet] == worst
    alone = [make_fr3_ensemble_controller("cem", lists[i], worst=worst[i]) for i in range(3)]
    for i in range(3):
        _configure(fleet[i], i, n=N)
        _configure(alone[i], i, n=N)
    for step in range(2):
        for i in range(3):
            cube = LIFTED if (i == 0 and step >= 1) else None
            _set_state(fleet[i], i, step, cube)
            _set_state(alone[i], i, step, cube)
        fleet.update_action()
        assert fleet._model_set.fr3 and fleet._model_set.info()["B"] == (6 if per_member else 2)
        for i in range(3):
            alone[i].update_action()
            _assert_same(_snap_ens(fleet[i]), _snap_ens(alone[i]), f"member {i} step {step}")
        assert [c.task.phase for c in fleet] == ([0, 1, 2] if step == 0 else [1, 1, 2])
    assert len({np.asarray(c.rewards).tobytes() for c in fleet}) == 3  # the members planned different problems


# ------------------------------------------------------------------------------------------------ 3. the randomised fleet
def test_randomized_fleet_equals_lone_randomized_controllers(gpu):
    """make_fr3_randomized_fleet("mppi", 3, [D0, D1, D2], blocks=4, weights per member): the members' own assignments, phases LIFT, MOVE, PLACE, member 0's cube lifted and
    member 2's assignment re-drawn between the two plan steps."""
    from judo_amd.fr3_randomized import FR3RandomizedController, make_fr3_randomized_controller
    from judo_amd.fr3_randomized_fleet import FR3RandomizedFleet, make_fr3_randomized_fleet

    descs = list(plants()[:3])
    weights = [[2, 1, 1], [1, 1, 2], [0, 1, 1]]
    fleet = make_fr3_randomized_fleet("mppi", 3, descs, blocks=4, weights=weights)
    assert isinstance(fleet, FR3RandomizedFleet) and all(type(c) is FR3RandomizedController for c in fleet)
    alone = [make_fr3_randomized_controller("mppi", descs, blocks=4, weights=weights[i]) for i in range(3)]
    assert [c.assignment for c in fleet] == [c.assignment for c in alone] and len({tuple(c.assignment) for c in fleet}) == 3
    for i in range(3):
        _configure(fleet[i], i, n=N)
        _configure(alone[i], i, n=N)
    for step in range(2):
        for i in range(3):
            cube = LIFTED if (i == 0 and step >= 1) else None
            _set_state(fleet[i], i, step, cube)
            _set_state(alone[i], i, step, cube)
        if step == 1:
            fleet[2].assignment = alone[2].assignment = [2, 0, 0, 1]
        fleet.update_action()
        for i in range(3):
            alone[i].update_action()
            s, t = _snap(fleet[i]), _snap(alone[i])
            s["plant_of_rollout"], t["plant_of_rollout"] = fleet[i].plant_of_rollout, alone[i].plant_of_rollout
            _assert_same(s, t, f"member {i} step {step}")
        assert [c.task.phase for c in fleet] == ([0, 1, 2] if step == 0 else [1, 1, 2])
    assert fleet[2].plant_of_rollout.tolist() == [2] * 12 + [0] * 24 + [1] * 12


# ------------------------------------------------------------------------------------------------ 4. who takes whom
def test_member_refusals(gpu):
    from judo_amd.ensemble_fleet import EnsembleFleet
    from judo_amd.fleet import ControllerFleet
    from judo_amd.fr3_ensemble import FR3EnsembleFleet, make_fr3_ensemble_controller
    from judo_amd.fr3_fleet import FR3Fleet, FR3PlantFleet
    from judo_amd.fr3_randomized import make_fr3_randomized_controller
    from judo_amd.fr3_randomized_fleet import FR3RandomizedFleet
    from judo_amd.randomized_fleet import RandomizedFleet

    d = plants()
    rn = make_fr3_randomized_controller("mppi", list(d[:2]))
    en = make_fr3_ensemble_controller("mppi", list(d[:2]))
    lone = _lone_on(d[0], "mppi")
    for fleet, members in ((ControllerFleet, [rn]), (EnsembleFleet, [rn]), (RandomizedFleet, [rn, rn]), (FR3Fleet, [lone, rn]), (FR3PlantFleet, [lone, rn])):
        with pytest.raises(ValueError, match="is an FR3RandomizedController.*no controller axis.*FR3RandomizedFleet"):
            fleet(members)
    for fleet, members in ((ControllerFleet, [en]), (EnsembleFleet, [en, en]), (RandomizedFleet, [en]), (FR3Fleet, [lone, en]), (FR3PlantFleet, [lone, en])):
        with pytest.raises(ValueError, match="is an FR3EnsembleController.*no controller axis.*FR3EnsembleFleet"):
            fleet(members)
    # the two new fleets take their own member class and nothing else
    assert len(FR3EnsembleFleet([en])) == 1 and len(FR3RandomizedFleet([rn])) == 1
    for other in (rn, lone):
        with pytest.raises(ValueError, match="fleet member 1 is a .*not an FR3EnsembleController"):
            FR3EnsembleFleet([en, other])
    for other in (en, lone):
        with pytest.raises(ValueError, match="fleet member 1 is a .*not an FR3RandomizedController"):
            FR3RandomizedFleet([rn, other])
    # one build of the kernel per launch
    ds = plants(True)
    with pytest.raises(ValueError, match="fleet member 1 differs from member 0 in self_collision"):
        FR3EnsembleFleet([en, make_fr3_ensemble_controller("mppi", list(ds[:2]), self_collision=True)])
    with pytest.raises(ValueError, match="fleet member 1 differs from member 0 in self_collision"):
        FR3RandomizedFleet([rn, make_fr3_randomized_controller("mppi", list(ds[:2]), self_collision=True)])
