"""The host side of fr3_pick on a model set (no GPU): the header, the ctypes table and the built library agree on the three new entries, the two modules import, the
issue's four plants are admitted as one set for both builds of the kernel, and the refusals that need no device."""

import ctypes
import functools
import os
import re

import pytest

from tests.conftest import ROOT

NEW = ("jh_fr3_model_set_create", "jh_plan_step_batch_phases_models", "jh_plan_step_randomized_phase")


def _prototype(header: str, name: str) -> list[str]:
    """The parameter names of `name`'s prototype in the header, in order."""
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", header)
    assert m, f"{name} is not declared"
    params = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",")
    return [re.findall(r"[A-Za-z_0-9]+", p)[-1] for p in params]


@functools.lru_cache(maxsize=None)
def plants(self_collision: bool = False):
    """D0..D3: the nominal fr3_pick description and three perturbed ones (cube mass and gripper gain; cube mass, pad friction and gain; the last link and the hand
    heavier on a slippery table)."""
    from judo_amd.models import scaled_description
    from judo_amd.tasks import FR3Pick

    d0 = FR3Pick(self_collision=self_collision).desc
    return (d0, scaled_description(d0, body_mass={"object": 0.7}, actuator_kp={None: 1.1}),
            scaled_description(d0, body_mass={"object": 1.4}, geom_friction={"box": 0.6}, actuator_kp={None: 0.9}),
            scaled_description(d0, body_mass={"fr3_link7": 1.2, "hand": 1.2}, geom_friction={"table": 0.5}))


def test_header_declares_the_three_entries():
    header = open(os.path.join(ROOT, "include", "judo_amd.h")).read()
    assert _prototype(header, "jh_fr3_model_set_create") == _prototype(header, "jh_model_set_create")
    phases = _prototype(header, "jh_plan_step_batch_phases")
    assert _prototype(header, "jh_plan_step_batch_phases_models") == ["set"] + phases[1:]  # `set` in place of `m`, B kept
    rnd = _prototype(header, "jh_plan_step_randomized")
    i = rnd.index("W")
    assert _prototype(header, "jh_plan_step_randomized_phase") == rnd[: i + 1] + ["phase"] + rnd[i + 1 :]


def test_ctypes_rows_match_and_the_library_exports_the_symbols():
    from judo_amd import _lib

    sig = _lib._SIGNATURES
    assert sig["jh_fr3_model_set_create"] == sig["jh_model_set_create"]
    assert sig["jh_plan_step_batch_phases_models"] == sig["jh_plan_step_batch_phases"]  # (a model and a set both travel as void pointers)
    res, args = sig["jh_plan_step_randomized"]
    i = 11  # set, blk_dev, blk_host, blk_bytes, o_nominal, o_sigma, o_tp, o_lohi, noise, ldn, W
    assert sig["jh_plan_step_randomized_phase"] == (res, args[:i] + [ctypes.c_int] + args[i:])
    built = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(built, name), name


def test_modules_import_without_a_device():
    from judo_amd import fr3_fleet, fr3_randomized
    from judo_amd.randomized import RandomizedController

    assert issubclass(fr3_fleet.FR3PlantFleet, fr3_fleet.FR3Fleet) and fr3_fleet.FR3PlantFleet._block_extra_words == 1
    assert issubclass(fr3_randomized.FR3RandomizedController, RandomizedController) and callable(fr3_randomized.make_fr3_randomized_controller)
    assert fr3_randomized.FR3RandomizedController._entry == "jh_plan_step_randomized_phase" and RandomizedController._entry == "jh_plan_step_randomized"


@pytest.mark.parametrize("self_collision", [False, True])
def test_the_four_plants_are_one_set(self_collision):
    """Equal sizes, header and int section byte for byte, and every perturbed image differs from D0's in its float section."""
    from judo_amd.ensemble import check_descriptions
    from judo_amd.models import image_sections

    blobs = check_descriptions(list(plants(self_collision)))
    assert len({len(b) for b in blobs}) == 1
    f0 = image_sections(blobs[0])[1]
    differ = [sum(x != y for x, y in zip(image_sections(b)[1], f0)) for b in blobs[1:]]
    assert all(n > 0 for n in differ) and len(set(differ)) == 3, differ


def test_refusals_without_a_device():
    from judo_amd.fr3_fleet import make_fr3_fleet
    from judo_amd.fr3_randomized import FR3RandomizedController, make_fr3_randomized_controller
    from judo_amd.config import ControllerConfig
    from judo_amd.models import scaled_description
    from judo_amd.randomized import check_task
    from judo_amd.tasks import FR3Pick, get_registered_tasks

    d = plants()
    with pytest.raises(ValueError, match="2 descriptions for a fleet of 3"):
        make_fr3_fleet("cem", 3, descriptions=list(d[:2]))
    with pytest.raises(ValueError, match="differs from the fleet in self_collision"):
        make_fr3_fleet("cem", 2, descriptions=[d[0], plants(True)[1]])
    with pytest.raises(ValueError, match="no fr3_pick description"):
        make_fr3_fleet("cem", 1, descriptions=[get_registered_tasks()["cartpole"][0]().desc])
    with pytest.raises(ValueError, match="fr3_pick has no randomised plan step"):  # the plain class keeps its refusal and names the new module
        check_task(FR3Pick())
    with pytest.raises(ValueError, match="fr3_randomized"):
        check_task(FR3Pick())
    check_task(FR3Pick(), fr3=True)
    with pytest.raises(ValueError, match="plans fr3_pick alone"):
        FR3RandomizedController(ControllerConfig(), get_registered_tasks()["cartpole"][0](), None, [d[0]])
    with pytest.raises(ValueError, match="differs from the task in self_collision"):
        make_fr3_randomized_controller("mppi", [d[0], d[1]], self_collision=True)
    with pytest.raises(ValueError, match="not found in optimizer registry"):
        make_fr3_randomized_controller("nope", [d[0]])
    with pytest.raises(ValueError, match="3 weights for M = 2"):
        make_fr3_randomized_controller("mppi", [d[0], d[1]], weights=[1, 1, 1])
    with pytest.raises(ValueError, match=r"assignment|blocks"):
        make_fr3_randomized_controller("mppi", [d[0], d[1]], blocks=0)
    other = dict(scaled_description(d[0]), geoms=d[0]["geoms"][:-1])  # a description with a geom less packs to another int section
    with pytest.raises(ValueError, match="member 1"):
        make_fr3_randomized_controller("mppi", [d[0], other])
