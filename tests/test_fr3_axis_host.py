"""The host side of the fr3 launch's controller axis (no GPU): the header, the ctypes table and the built library agree on the three new entries, the two modules import
with the classes on their bases, and the factories' refusals that need no device."""

import ctypes
import os

import pytest

from tests.conftest import ROOT
from tests.test_fr3_plants_host import _prototype, plants

NEW = ("jh_plan_step_ensemble_phase", "jh_plan_step_ensemble_batch_phases", "jh_plan_step_randomized_batch_phases")


def _with(params, behind, name):
    i = params.index(behind)
    return params[: i + 1] + [name] + params[i + 1 :]


def test_header_declares_the_three_entries():
    header = open(os.path.join(ROOT, "include", "judo_amd.h")).read()
    assert _prototype(header, "jh_plan_step_ensemble_phase") == _with(_prototype(header, "jh_plan_step_ensemble"), "W", "phase")
    assert _prototype(header, "jh_plan_step_ensemble_batch_phases") == _with(_prototype(header, "jh_plan_step_ensemble_batch"), "o_lohi", "o_phase")
    assert _prototype(header, "jh_plan_step_randomized_batch_phases") == _with(_prototype(header, "jh_plan_step_randomized_batch"), "o_lohi", "o_phase")


def test_ctypes_rows_match_and_the_library_exports_the_symbols():
    from judo_amd import _lib

    sig = _lib._SIGNATURES
    res, args = sig["jh_plan_step_ensemble"]
    i = 11  # set, blk_dev, blk_host, blk_bytes, o_nominal, o_sigma, o_tp, o_lohi, noise, ldn, W
    assert sig["jh_plan_step_ensemble_phase"] == (res, args[:i] + [ctypes.c_int] + args[i:])
    i = 11  # set, B, M, blk_dev, blk_host, blk_bytes, blk_stride_bytes, o_nominal, o_sigma, o_tp, o_lohi
    for old, new in (("jh_plan_step_ensemble_batch", "jh_plan_step_ensemble_batch_phases"), ("jh_plan_step_randomized_batch", "jh_plan_step_randomized_batch_phases")):
        res, args = sig[old]
        assert sig[new] == (res, args[:i] + [ctypes.c_int] + args[i:]), new
    built = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(built, name), name


def test_modules_import_without_a_device():
    from judo_amd import fr3_ensemble, fr3_randomized_fleet
    from judo_amd.ensemble import EnsembleController
    from judo_amd.ensemble_fleet import EnsembleFleet
    from judo_amd.fr3_randomized import FR3RandomizedController
    from judo_amd.randomized_fleet import RandomizedFleet

    assert issubclass(fr3_ensemble.FR3EnsembleController, EnsembleController)
    assert fr3_ensemble.FR3EnsembleController._entry == "jh_plan_step_ensemble_phase" and EnsembleController._entry == "jh_plan_step_ensemble"
    assert issubclass(fr3_ensemble.FR3EnsembleFleet, EnsembleFleet) and fr3_ensemble.FR3EnsembleFleet._block_extra_words == 1
    assert issubclass(fr3_randomized_fleet.FR3RandomizedFleet, RandomizedFleet) and fr3_randomized_fleet.FR3RandomizedFleet._block_extra_words == 1
    assert FR3RandomizedController._entry == "jh_plan_step_randomized_phase"
    assert not EnsembleFleet._block_extra_words and not RandomizedFleet._block_extra_words
    assert callable(fr3_ensemble.make_fr3_ensemble_controller) and callable(fr3_ensemble.make_fr3_ensemble_fleet) and callable(fr3_randomized_fleet.make_fr3_randomized_fleet)


def test_refusals_without_a_device():
    from judo_amd.config import ControllerConfig
    from judo_amd.ensemble import check_task, make_ensemble_controller
    from judo_amd.fr3_ensemble import FR3EnsembleController, make_fr3_ensemble_controller, make_fr3_ensemble_fleet
    from judo_amd.fr3_randomized_fleet import make_fr3_randomized_fleet
    from judo_amd.randomized_fleet import make_randomized_fleet
    from judo_amd.tasks import FR3Pick, get_registered_tasks

    d, ds = plants(), plants(True)
    for make in (lambda o: make_fr3_ensemble_controller(o, [d[0], d[1]]), lambda o: make_fr3_ensemble_fleet(o, 2, [d[0], d[1]]), lambda o: make_fr3_randomized_fleet(o, 2, [d[0], d[1]])):
        with pytest.raises(ValueError, match="not found in optimizer registry"):
            make("nope")
    with pytest.raises(ValueError, match="description 1 differs from the task in self_collision"):
        make_fr3_ensemble_controller("mppi", [ds[0], d[1]], self_collision=True)
    with pytest.raises(ValueError, match="description 0 differs from the task in self_collision"):
        make_fr3_ensemble_controller("mppi", [ds[0], ds[1]])
    with pytest.raises(ValueError, match="fleet member 0: description 1 differs from the task in self_collision"):
        make_fr3_ensemble_fleet("mppi", 2, [d[0], ds[1]])
    with pytest.raises(ValueError, match="fleet member 1: description 0 differs from the task in self_collision"):
        make_fr3_randomized_fleet("mppi", 2, [[d[0], d[1]], [ds[0], ds[1]]])
    with pytest.raises(ValueError, match="worst = 3 outside"):
        make_fr3_ensemble_fleet("mppi", 2, [d[0], d[1]], worst=3)
    with pytest.raises(ValueError, match="3 lists of descriptions for a fleet of 2"):
        make_fr3_ensemble_fleet("mppi", 2, [[d[0]], [d[1]], [d[2]]])
    with pytest.raises(ValueError, match="plans fr3_pick alone"):
        FR3EnsembleController(ControllerConfig(), get_registered_tasks()["cartpole"][0](), None, [d[0]])
    # the plain classes keep their refusals and name the new factories
    with pytest.raises(ValueError, match="fr3_pick has no ensemble plan step.*make_fr3_ensemble_controller"):
        check_task(FR3Pick())
    check_task(FR3Pick(), fr3=True)
    with pytest.raises(ValueError, match="fr3_pick has no ensemble plan step"):
        make_ensemble_controller("fr3_pick", "mppi", [d[0], d[1]])
    with pytest.raises(ValueError, match="fr3_pick has no randomised plan step.*make_fr3_randomized_fleet"):
        make_randomized_fleet("fr3_pick", "mppi", 2, [d[0], d[1]])
