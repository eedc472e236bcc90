"""The device-free parts of judo_amd/fr3_materialized.py and of the arm's materialise launch on plants: the admission of task and descriptions, the validation of
`worst` and of the blocks, the fleets' refusal by name, the hints of the fused fr3 classes, the boundary's symbol table."""

import copy
import os
import re
import types

import pytest

from tests.test_fr3_plants_host import _prototype, plants

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "jh_fr3_rollout_materialize_plants"


def _task(name):
    from judo_amd.tasks import get_registered_tasks

    return get_registered_tasks()[name][0]()


def test_the_makers_refuse_other_families_without_a_device():
    from judo_amd.fr3_materialized import check_fr3_task, make_fr3_materialized_ensemble_controller, make_fr3_materialized_randomized_controller
    from judo_amd.tasks import FR3Pick

    cart, spot = _task("cartpole"), _task("spot_navigate")
    with pytest.raises(ValueError, match=r"plans fr3_pick alone \(Cartpole, family cartpole\).*jh_fr3_rollout_materialize_plants.*make_materialized_ensemble_controller"):
        make_fr3_materialized_ensemble_controller("cartpole", "mppi", [cart.desc, cart.desc])
    with pytest.raises(ValueError, match=r"plans fr3_pick alone.*make_materialized_randomized_controller"):
        make_fr3_materialized_randomized_controller(_task("leap_cube"), "cem", [_task("leap_cube").desc])
    with pytest.raises(ValueError, match=r"Spot policy tasks.*make_spot_ensemble_controller"):
        make_fr3_materialized_ensemble_controller("spot_navigate", "mppi", [spot.desc, spot.desc])
    with pytest.raises(ValueError, match=r"Spot policy tasks.*make_spot_randomized_controller"):
        make_fr3_materialized_randomized_controller(spot, "mppi", [spot.desc, spot.desc])
    with pytest.raises(ValueError, match="not found in task registry"):
        make_fr3_materialized_ensemble_controller("no_such_task", "mppi", [plants()[0]])
    with pytest.raises(ValueError, match="not found in optimizer registry"):
        make_fr3_materialized_ensemble_controller("fr3_pick", "no_such_optimizer", [plants()[0]])

    class Plugin(FR3Pick):
        def reward(self, states, sensors, controls, system_metadata=None):
            return -(states[..., :3] ** 2).sum(-1).sum(-1)

    for t in (FR3Pick(), FR3Pick(self_collision=True), Plugin()):
        check_fr3_task(t)
        check_fr3_task(t, "randomized")


def test_descriptions_pass_the_fr3_plant_admission():
    """The float section alone may differ, and every description is of the task's build: another topology is refused naming the member and the section, members mixed in
    self_collision naming the description -- before a device is touched."""
    from judo_amd.config import ControllerConfig
    from judo_amd.fr3_materialized import FR3MaterializedEnsembleController, FR3MaterializedRandomizedController, admit
    from judo_amd.tasks import FR3Pick

    d, ds = plants(), plants(True)
    assert len(admit(FR3Pick(), list(d), "ensemble")) == 4 and len(admit(FR3Pick(self_collision=True), list(ds), "randomized")) == 4
    edited = copy.deepcopy(d[0])
    edited["geoms"] = edited["geoms"][:-1]  # one geom fewer: the header and the int section move with the float section
    for cls in (FR3MaterializedEnsembleController, FR3MaterializedRandomizedController):
        with pytest.raises(ValueError, match=r"ensemble member 1 has another model image than member 0: the (header|float section|int section)"):
            cls(ControllerConfig(), FR3Pick(), None, [d[0], edited])
        with pytest.raises(ValueError, match=r"ensemble member 1 has another model image than member 0"):
            cls(ControllerConfig(), FR3Pick(), None, [d[0], _task("cartpole").desc])
        with pytest.raises(ValueError, match=r"description 1 differs from the task in self_collision"):
            cls(ControllerConfig(), FR3Pick(), None, [d[0], ds[1]])
        with pytest.raises(ValueError, match=r"description 0 differs from the task in self_collision: derive the descriptions from FR3Pick\(self_collision=True\)"):
            cls(ControllerConfig(), FR3Pick(self_collision=True), None, [d[0], ds[1]])
        with pytest.raises(ValueError, match="at least one description"):
            cls(ControllerConfig(), FR3Pick(), None, [], **({"blocks": 1} if cls is FR3MaterializedRandomizedController else {}))


def test_worst_and_blocks_are_validated_before_a_device_is_touched():
    from judo_amd.config import ControllerConfig
    from judo_amd.fr3_materialized import FR3MaterializedEnsembleController, FR3MaterializedRandomizedController
    from judo_amd.tasks import FR3Pick

    two = list(plants()[:2])
    for worst in (0, 3, -1):
        with pytest.raises(ValueError, match=rf"worst = {worst} outside \[1, M = 2\]"):
            FR3MaterializedEnsembleController(ControllerConfig(), FR3Pick(), None, two, worst=worst)
    with pytest.raises(ValueError, match="3 weights for M = 2 plants"):
        FR3MaterializedRandomizedController(ControllerConfig(), FR3Pick(), None, two, blocks=4, weights=[1, 1, 1])
    with pytest.raises(ValueError, match="0 blocks"):
        FR3MaterializedRandomizedController(ControllerConfig(), FR3Pick(), None, two, blocks=0)
    # blocks that do not divide num_rollouts: the plan step's first check, in front of anything on the device (an instance without a device: the check reads these alone)
    c = object.__new__(FR3MaterializedRandomizedController)
    c.optimizer = types.SimpleNamespace(config=types.SimpleNamespace(num_rollouts=16), num_rollouts=16)
    c._assignment, c._assignment_used = [0, 1, 0], None
    with pytest.raises(ValueError, match=r"num_rollouts % blocks != 0: 16 rollouts do not split into 3 equal blocks"):
        c.update_action()
    with pytest.raises(ValueError, match=r"num_rollouts % blocks != 0"):
        c.plant_of_rollout


def test_the_classes_are_thin_subclasses():
    """`_admit` alone is overridden: everything else is the classes' of judo_amd/materialized.py, the fleets' mark included."""
    from judo_amd import fr3_materialized as fm
    from judo_amd.materialized import MaterializedEnsembleController, MaterializedRandomizedController

    for cls, base in ((fm.FR3MaterializedEnsembleController, MaterializedEnsembleController), (fm.FR3MaterializedRandomizedController, MaterializedRandomizedController)):
        assert cls.__bases__ == (base,) and cls._materialized_plants is True
        assert [k for k in vars(cls) if not k.startswith("__")] == ["_admit"], vars(cls).keys()


def test_the_boundary_lists_the_new_symbol():
    import ctypes

    from judo_amd import _lib

    header = open(os.path.join(ROOT, "include", "judo_amd.h")).read()
    declared = set(re.findall(r"\b(jh_[a-z_0-9]+)\s*\(", header))
    assert NAME in _lib.EXPORTED_SYMBOLS and NAME in declared
    assert _prototype(header, NAME) == _prototype(header, "jh_rollout_materialize_plants")
    assert _lib._SIGNATURES[NAME] == _lib._SIGNATURES["jh_rollout_materialize_plants"]
    assert getattr(_lib.lib(), NAME).argtypes == _lib._SIGNATURES[NAME][1]
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), NAME)
    assert NAME in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def test_the_fleets_refuse_the_new_classes_by_name():
    """Every fleet's `_check_member` begins with fleet.refuse_fr3_randomized, which refuses a member that carries the classes' mark."""
    import inspect

    from judo_amd import ensemble_fleet, fleet, fr3_fleet, fr3_randomized_fleet, randomized_fleet
    from judo_amd.fr3_materialized import FR3MaterializedEnsembleController, FR3MaterializedRandomizedController

    for cls in (FR3MaterializedEnsembleController, FR3MaterializedRandomizedController):
        member = object.__new__(cls)  # (no device: the refusal reads the class alone)
        with pytest.raises(ValueError, match=rf"fleet member 1 is a {cls.__name__} .*plant 0 alone.*No fleet takes such a member"):
            fleet.refuse_fr3_randomized(1, member, None)
        with pytest.raises(ValueError, match=rf"fleet member 0 is a {cls.__name__}"):
            fleet.ControllerFleet._check_member(object.__new__(fleet.ControllerFleet), 0, member, member)
    for mod in (fleet, ensemble_fleet, randomized_fleet, fr3_fleet, fr3_randomized_fleet):
        src = inspect.getsource(mod)
        assert "refuse_fr3_randomized(i, c, self)" in src or "super()._check_member(i, c, first)" in src, mod.__name__


def test_the_hints_name_the_new_makers():
    """The fused fr3 classes refuse a plugin configuration as before; behind their text they name the maker that serves it.  `materialized.check_task` keeps its text
    and adds the new makers behind it."""
    from judo_amd.fr3_ensemble import FR3EnsembleController, materialized_hint
    from judo_amd.fr3_randomized import FR3RandomizedController
    from judo_amd.materialized import check_task
    from judo_amd.tasks import FR3Pick

    for cls, kind in ((FR3EnsembleController, "ensemble"), (FR3RandomizedController, "randomized")):
        c = object.__new__(cls)
        assert f"judo_amd.fr3_materialized.make_fr3_materialized_{kind}_controller" in c._hint("the running normaliser: its moments need the materialise path")
        assert f"make_fr3_materialized_{kind}_controller" in c._hint("") and "make_materialized_" not in c._hint("")
        assert c._hint("a process group or force_shard_path: the sharded path has no ensemble form") == "" and c._hint("keep_candidates: no candidate knots") == ""
        c.optimizer = types.SimpleNamespace(config=types.SimpleNamespace(num_rollouts=16))
        c.fused_update, c._assignment = False, [0]
        c.task = FR3Pick()
        with pytest.raises(ValueError, match=rf"uses_fused_cost is false.*make_fr3_materialized_{kind}_controller"):
            c.update_action()
        with pytest.raises(ValueError, match=rf"fr3_pick has no materialise launch on plants: the cooperative arm kernel's batched instantiations are fused launches.*"
                                             rf"make_fr3_{kind}_controller.*make_fr3_materialized_{kind}_controller"):
            check_task(FR3Pick(), kind)
    assert materialized_hint("", "ensemble").startswith(".  ")
