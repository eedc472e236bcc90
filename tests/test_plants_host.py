"""The worst-case and assignment pieces of judo_amd/plants.py on a stub without a device, and that the concrete controllers take these members from the one place."""

import re
import types

import pytest


def _stub(num_rollouts=12):
    """The two pieces over what they read of a controller: three descriptions, the optimizer's rollout count, and an `update_action` to stand behind the guard."""
    from judo_amd.plants import Assignment, WorstCase

    class Plain:
        updates = 0

        def update_action(self):
            self.updates += 1

    class Stub(WorstCase, Assignment, Plain):
        optimizer_cfg = property(lambda self: self.optimizer.config)

    s = Stub()
    s._descriptions = [{}, {}, {}]
    s.optimizer = types.SimpleNamespace(num_rollouts=num_rollouts, config=types.SimpleNamespace(num_rollouts=num_rollouts))
    return s


def test_worst_is_validated_when_made_and_when_set():
    s = _stub()
    s._init_worst(None, 3)
    assert s.worst == 3 and s._member_costs is None  # (None: the mean)
    with pytest.raises(RuntimeError, match="member_costs needs a completed update_action"):
        s.member_costs
    s.worst = 1
    assert s.worst == 1
    for bad in (4, 0, -1):
        with pytest.raises(ValueError, match=re.escape(f"worst = {bad} outside [1, M = 3]")):
            s.worst = bad
        with pytest.raises(ValueError, match=re.escape(f"worst = {bad} outside [1, M = 3]")):
            _stub()._init_worst(bad, 3)
    assert s.worst == 1  # (a refused value changes nothing)


def test_assignment_and_weights_are_validated():
    s = _stub()
    s._init_assignment(None, None, 3)
    assert s.assignment == [0, 1, 2] and s.blocks == 3 and s._assignment_used is None  # (the default: block g on plant g % M)
    with pytest.raises(ValueError, match=re.escape("assignment[1] = 3 outside [0, M = 3)")):
        s.assignment = [0, 3, 1]
    with pytest.raises(ValueError, match="2 weights for M = 3 plants"):
        s.set_weights([1, 1])
    with pytest.raises(ValueError, match="2 weights for M = 3 plants"):
        _stub()._init_assignment(4, [1, 1], 3)
    assert s.assignment == [0, 1, 2]
    s.set_weights([2, 1, 1], blocks=4)
    assert s.assignment == [0, 0, 1, 2] and s.blocks == 4
    s.set_weights([0, 1, 1])  # (`blocks` None keeps the number of blocks)
    assert s.assignment == [1, 1, 2, 2]
    got = s.assignment
    got[0] = 2
    assert s.assignment == [1, 1, 2, 2]  # (a copy is handed out)


def test_plant_of_rollout_before_a_first_plan_step():
    s = _stub()
    s._init_assignment(4, [2, 1, 1], 3)
    assert s.plant_of_rollout.tolist() == [0] * 6 + [1] * 3 + [2] * 3  # (of the next plan step: the assignment in force over the optimizer's num_rollouts)
    s.assignment = [2, 0]
    assert s.plant_of_rollout.tolist() == [2] * 6 + [0] * 6


def test_blocks_that_do_not_divide_num_rollouts_stop_the_plan_step():
    s = _stub(num_rollouts=10)
    s._init_assignment(4, None, 3)
    with pytest.raises(ValueError, match=re.escape("num_rollouts % blocks != 0: 10 rollouts do not split into 4 equal blocks")):
        s.update_action()
    with pytest.raises(ValueError, match=re.escape("num_rollouts % blocks != 0")):
        s.plant_of_rollout
    assert s.updates == 0
    s.optimizer.config.num_rollouts = 12
    s.update_action()
    assert s.updates == 1  # (the guard passes the call on)


def test_the_controllers_take_these_members_from_the_one_place():
    from judo_amd import plants
    from judo_amd.ensemble import EnsembleController
    from judo_amd.fr3_ensemble import FR3EnsembleController
    from judo_amd.fr3_materialized import FR3MaterializedEnsembleController, FR3MaterializedRandomizedController
    from judo_amd.fr3_randomized import FR3RandomizedController
    from judo_amd.materialized import MaterializedEnsembleController, MaterializedRandomizedController
    from judo_amd.randomized import RandomizedController
    from judo_amd.spot_plants import SpotEnsembleController, SpotRandomizedController

    worst_case = (EnsembleController, FR3EnsembleController, MaterializedEnsembleController, FR3MaterializedEnsembleController, SpotEnsembleController)
    assigned = (RandomizedController, FR3RandomizedController, MaterializedRandomizedController, FR3MaterializedRandomizedController, SpotRandomizedController)
    for cls in worst_case:
        for name in ("worst", "member_costs", "member_rewards", "_member_cost_rows"):
            assert getattr(cls, name) is getattr(plants.WorstCase, name), (cls.__name__, name)
        assert not hasattr(cls, "assignment")
    for cls in assigned:
        for name in ("blocks", "assignment", "set_weights", "plant_of_rollout", "plant_rewards"):
            assert getattr(cls, name) is getattr(plants.Assignment, name), (cls.__name__, name)
        assert not hasattr(cls, "worst")
    for cls in worst_case + assigned:  # (the `GpuModelSet` users and the Spot pair: one bounds check and one bookkeeping, the set's own step behind `_replace_plant`)
        for name in ("set_member", "descriptions", "num_members"):
            assert getattr(cls, name) is getattr(plants.PlantSet, name), (cls.__name__, name)
        gpu_set = not cls.__name__.startswith("Spot")
        assert (cls._replace_plant is plants.GpuPlantSet._replace_plant) == gpu_set and issubclass(cls, plants.GpuPlantSet) == gpu_set
    for cls in (EnsembleController, RandomizedController, FR3EnsembleController, FR3RandomizedController):
        for name in ("_plan_step", "_iteration_shape", "_refusal"):
            assert getattr(cls, name) is getattr(plants.FusedPlantController, name), (cls.__name__, name)
    assert EnsembleController._ensemble_refusal is RandomizedController._randomized_refusal is plants.FusedPlantController._refusal
    # the guard of the assignment runs behind the fused pair's own and in front of the controller's
    mro = RandomizedController.__mro__
    assert mro.index(plants.FusedPlantController) < mro.index(plants.Assignment) < mro.index(RandomizedController.__mro__[-2])
