"""The device-free parts of judo_amd/materialized.py and of the plants rollout: the admission of the descriptions, the validation of `worst`, tables and weights, the
refusals by task that are raised before any model is made, the fleets' refusal by name, the boundary's symbol table."""

import copy
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _task(name):
    from judo_amd.tasks import get_registered_tasks

    return get_registered_tasks()[name][0]()


def test_descriptions_pass_the_ensemble_admission():
    """The float section alone may differ: scaled plants pass, another topology is refused naming the member and the section -- before a device is touched."""
    from judo_amd.config import ControllerConfig
    from judo_amd.ensemble import check_descriptions
    from judo_amd.materialized import MaterializedEnsembleController, MaterializedRandomizedController
    from judo_amd.models import scaled_description

    base = _task("leap_cube").desc
    assert len(check_descriptions([base, scaled_description(base, body_mass={"cube": 1.5}, geom_friction={"cube": 0.6})])) == 2
    edited = copy.deepcopy(base)
    edited["excludes"][0] = [6, 10]  # another <exclude> pair moves the pair lists of the int section and nothing else
    for cls in (MaterializedEnsembleController, MaterializedRandomizedController):
        with pytest.raises(ValueError, match=r"ensemble member 1 has another model image than member 0: the int section"):
            cls(ControllerConfig(), _task("leap_cube"), None, [base, edited])
        with pytest.raises(ValueError, match=r"ensemble member 1 has another model image than member 0: the (header|float section|int section)"):
            cls(ControllerConfig(), _task("cartpole"), None, [_task("cartpole").desc, _task("cylinder_push").desc])
        with pytest.raises(ValueError, match="at least one description"):
            cls(ControllerConfig(), _task("cartpole"), None, [], **({"blocks": 1} if cls is MaterializedRandomizedController else {}))
        with pytest.raises(ValueError, match="33 members.*JH_MAX_ENSEMBLE"):
            cls(ControllerConfig(), _task("cartpole"), None, [_task("cartpole").desc] * 33, **({"blocks": 1} if cls is MaterializedRandomizedController else {}))


def test_worst_assignment_and_weights_are_validated_before_a_device_is_touched():
    from judo_amd.config import ControllerConfig
    from judo_amd.materialized import MaterializedEnsembleController, MaterializedRandomizedController

    t = _task("cartpole")
    two = [t.desc, t.desc]
    for worst in (0, 3, -1):
        with pytest.raises(ValueError, match=rf"worst = {worst} outside \[1, M = 2\]"):
            MaterializedEnsembleController(ControllerConfig(), t, None, two, worst=worst)
    with pytest.raises(ValueError, match="3 weights for M = 2 plants"):
        MaterializedRandomizedController(ControllerConfig(), t, None, two, blocks=4, weights=[1, 1, 1])
    with pytest.raises(ValueError, match="weights must be non-negative"):
        MaterializedRandomizedController(ControllerConfig(), t, None, two, blocks=4, weights=[1, -1])
    with pytest.raises(ValueError, match="0 blocks"):
        MaterializedRandomizedController(ControllerConfig(), t, None, two, blocks=0)
    with pytest.raises(ValueError, match="65 blocks.*JH_MAX_PLANT_BLOCKS"):
        MaterializedRandomizedController(ControllerConfig(), t, None, two, blocks=65)


def test_the_plant_table_of_the_backend_is_validated_on_the_host():
    from judo_amd import _lib
    from judo_amd.rollout_backend import check_plant_table

    assert check_plant_table([2, 0, 2], 3) == [2, 0, 2] and check_plant_table(range(3), 3) == [0, 1, 2]
    with pytest.raises(ValueError, match=r"plant_of_block\[1\] = 3 outside \[0, M = 3\): block 1"):
        check_plant_table([0, 3], 3)
    with pytest.raises(ValueError, match=r"plant_of_block\[0\] = -1"):
        check_plant_table([-1], 3)
    with pytest.raises(ValueError, match=r"plant_of_block\[0\] = 0.5"):
        check_plant_table([0.5], 3)
    with pytest.raises(ValueError, match=r"plant_of_block\[0\] = True"):
        check_plant_table([True], 3)
    with pytest.raises(ValueError, match="a table of 0 blocks"):
        check_plant_table([], 3)
    with pytest.raises(ValueError, match=rf"a table of {_lib.MAX_FLEET_PLANT_BLOCKS + 1} blocks.*JH_MAX_FLEET_PLANT_BLOCKS"):
        check_plant_table([0] * (_lib.MAX_FLEET_PLANT_BLOCKS + 1), 3)


def test_the_makers_refuse_spot_and_fr3_without_a_device():
    from judo_amd.materialized import check_task, make_materialized_ensemble_controller, make_materialized_randomized_controller

    spot, fr3 = _task("spot_navigate"), _task("fr3_pick")
    with pytest.raises(ValueError, match=r"Spot policy tasks.*make_spot_ensemble_controller"):
        make_materialized_ensemble_controller("spot_navigate", "mppi", [spot.desc, spot.desc])
    with pytest.raises(ValueError, match=r"Spot policy tasks.*make_spot_randomized_controller"):
        make_materialized_randomized_controller("spot_navigate", "mppi", [spot.desc, spot.desc])
    with pytest.raises(ValueError, match=r"fr3_pick has no materialise launch on plants: the cooperative arm kernel's batched instantiations are fused launches.*make_fr3_ensemble_controller"):
        make_materialized_ensemble_controller(fr3, "cem", [fr3.desc])
    with pytest.raises(ValueError, match=r"fr3_pick has no materialise launch on plants.*make_fr3_randomized_controller"):
        make_materialized_randomized_controller("fr3_pick", "cem", [fr3.desc])
    with pytest.raises(ValueError, match="not found in task registry"):
        make_materialized_ensemble_controller("no_such_task", "mppi", [spot.desc])
    with pytest.raises(ValueError, match="not found in optimizer registry"):
        make_materialized_ensemble_controller("cartpole", "no_such_optimizer", [_task("cartpole").desc])
    for name in ("cartpole", "cylinder_push", "leap_cube", "leap_cube_down", "caltech_leap_cube"):
        check_task(_task(name))


def test_the_fused_classes_name_the_new_makers():
    """The refusals of EnsembleController and RandomizedController stand; behind their text they name the maker that serves the configuration (never for fr3_pick)."""
    from judo_amd.ensemble import _materialized_hint as ensemble_hint
    from judo_amd.randomized import _materialized_hint as randomized_hint

    assert "make_materialized_ensemble_controller" in ensemble_hint("the running normaliser: its moments need the materialise path")
    assert "make_materialized_randomized_controller" in randomized_hint("a plugin reward, hook or optimizer (uses_fused_cost is false)")
    for hint in (ensemble_hint, randomized_hint):
        assert hint("a process group or force_shard_path: the sharded path has no ensemble form") == "" and hint("keep_candidates: no candidate knots") == ""
        assert hint("a plugin reward", True) == ""


def test_the_fleets_refuse_the_new_classes_by_name():
    """Every fleet's `_check_member` begins with fleet.refuse_fr3_randomized, which refuses a member that carries the classes' mark."""
    import inspect

    from judo_amd import ensemble_fleet, fleet, fr3_fleet, randomized_fleet
    from judo_amd.materialized import MaterializedEnsembleController, MaterializedRandomizedController

    for cls in (MaterializedEnsembleController, MaterializedRandomizedController):
        assert cls._materialized_plants is True
        member = object.__new__(cls)  # (no device: the refusal reads the class alone)
        with pytest.raises(ValueError, match=rf"fleet member 1 is a {cls.__name__} \(judo_amd.materialized\).*jh_rollout_materialize_plants.*plant 0 alone"):
            fleet.refuse_fr3_randomized(1, member, None)
        with pytest.raises(ValueError, match=rf"fleet member 0 is a {cls.__name__}"):
            fleet.ControllerFleet._check_member(object.__new__(fleet.ControllerFleet), 0, member, member)
    for mod in (fleet, ensemble_fleet, randomized_fleet, fr3_fleet):
        assert "refuse_fr3_randomized(i, c, self)" in inspect.getsource(mod), mod.__name__


def test_the_boundary_lists_the_new_symbol():
    from judo_amd import _lib

    header = open(os.path.join(ROOT, "include", "judo_amd.h")).read()
    declared = set(re.findall(r"\b(jh_[a-z_0-9]+)\s*\(", header))
    name = "jh_rollout_materialize_plants"
    assert name in _lib.EXPORTED_SYMBOLS and name in declared
    assert getattr(_lib.lib(), name).argtypes == _lib._SIGNATURES[name][1]
    assert name in open(os.path.join(ROOT, "INTEGRATION.md")).read()
