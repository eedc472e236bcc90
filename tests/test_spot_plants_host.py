"""The host side of the Spot controllers on perturbed plants (judo_amd/spot_plants.py, judo_amd/tree_model.py): the admission rule of a set of tree images, the
validation of assignment, weights and `worst`, the refusals that come before any device is touched, and the C boundary's new names.  No GPU."""

import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW_SYMBOLS = ("jh_tree_set_create", "jh_tree_set_update", "jh_tree_set_info", "jh_tree_set_stats", "jh_tree_set_destroy", "jh_tree_substeps_plants", "jh_policy_rollout_plants")


def _base(name):
    from judo_amd.models import load_description, spot_box_description, spot_tire_description

    return {"spot": lambda: load_description("spot"), "spot_box": spot_box_description, "spot_tire": spot_tire_description}[name]()


def _scalings(desc):
    """The three kinds of scaling on names the description has: the last body with a mass, the last geom in front of the ground plane, every actuator."""
    body = [b["name"] for b in desc["bodies"] if b.get("mass", 0) > 0][-1]
    geom = [g["name"] for g in desc["geoms"] if g.get("name") and g["type"] != "plane"][-1]
    return [dict(body_mass={body: 1.7}), dict(geom_friction={geom: 0.6}), dict(actuator_kp={None: 1.2}), dict(body_mass={body: 1.7}, geom_friction={geom: 0.6}, actuator_kp={None: 1.2})]


@pytest.mark.parametrize("name", ["spot", "spot_box", "spot_tire"])
def test_scaled_descriptions_are_admitted_and_differ_in_the_float_section_alone(name):
    from judo_amd.models import scaled_description
    from judo_amd.tree_model import check_tree_descriptions, tree_image_sections

    base = _base(name)
    members = [base] + [scaled_description(base, **kw) for kw in _scalings(base)]
    blobs = check_tree_descriptions(members)
    assert len(blobs) == len(members) and all(isinstance(b, bytes) for b in blobs)
    h0, f0, i0 = tree_image_sections(blobs[0])
    assert len(h0) == 16 and len(h0) + len(f0) + len(i0) == len(blobs[0])
    for b in blobs[1:]:
        h, f, i = tree_image_sections(b)
        assert h == h0 and i == i0 and len(f) == len(f0)
        assert f != f0  # (a scaling that changed nothing would test nothing)
        ndiff = int((np.frombuffer(f, dtype=np.uint32) != np.frombuffer(f0, dtype=np.uint32)).sum())
        assert 1 <= ndiff <= 200  # a few masses, inertias, friction coefficients or gains: never the layout


def test_the_box_scaling_of_the_gpu_tests_is_admitted():
    from judo_amd.models import scaled_description
    from judo_amd.tree_model import check_tree_descriptions

    base = _base("spot_box")
    check_tree_descriptions([base, scaled_description(base, body_mass={"box_body": 1.7}, geom_friction={"box_collision": 0.6}, actuator_kp={None: 1.2})])


def test_a_removed_geom_is_refused_naming_the_section():
    import copy

    from judo_amd.tree_model import check_tree_descriptions

    base = _base("spot_box")
    cut = copy.deepcopy(base)
    victim = next(k for k, g in enumerate(cut["geoms"]) if g.get("name") == "right_jaw_collision")
    del cut["geoms"][victim]
    with pytest.raises(ValueError, match=r"Spot plant 2 has another model image than plant 0: the (header|float section|int section)"):
        check_tree_descriptions([base, base, cut])


def test_a_mixed_list_is_refused():
    from judo_amd.tree_model import check_tree_descriptions

    with pytest.raises(ValueError, match=r"Spot plant 1 has another model image than plant 0: the header"):
        check_tree_descriptions([_base("spot"), _base("spot_box")])
    with pytest.raises(ValueError, match="at least one"):
        check_tree_descriptions([])
    with pytest.raises(ValueError, match="33 Spot plants.*JH_MAX_ENSEMBLE"):
        check_tree_descriptions([_base("spot")] * 33)


def _spot_task():
    from judo_amd.tasks import get_registered_tasks

    return get_registered_tasks()["spot_box_push"][0]()


def test_worst_assignment_and_weights_are_validated_before_a_device_is_touched():
    from judo_amd.config import ControllerConfig
    from judo_amd.spot_plants import SpotEnsembleController, SpotRandomizedController

    t = _spot_task()
    two = [t.desc, t.desc]
    for worst in (0, 3, -1):
        with pytest.raises(ValueError, match=rf"worst = {worst} outside \[1, M = 2\]"):
            SpotEnsembleController(ControllerConfig(), t, None, two, worst=worst)
    with pytest.raises(ValueError, match="3 weights for M = 2 plants"):
        SpotRandomizedController(ControllerConfig(), t, None, two, blocks=4, weights=[1, 1, 1])
    with pytest.raises(ValueError, match="weights must be non-negative"):
        SpotRandomizedController(ControllerConfig(), t, None, two, blocks=4, weights=[1, -1])
    with pytest.raises(ValueError, match="0 blocks"):
        SpotRandomizedController(ControllerConfig(), t, None, two, blocks=0)
    with pytest.raises(ValueError, match="65 blocks.*JH_MAX_PLANT_BLOCKS"):
        SpotRandomizedController(ControllerConfig(), t, None, two, blocks=65)


def test_the_makers_refuse_other_tasks_without_a_device():
    from judo_amd.spot_plants import make_spot_ensemble_controller, make_spot_randomized_controller
    from judo_amd.tasks import get_registered_tasks

    desc = get_registered_tasks()["cartpole"][0]().desc
    with pytest.raises(ValueError, match=r"cartpole does not use the locomotion policy.*make_ensemble_controller"):
        make_spot_ensemble_controller("cartpole", "mppi", [desc, desc])
    with pytest.raises(ValueError, match=r"cartpole does not use the locomotion policy.*make_randomized_controller"):
        make_spot_randomized_controller("cartpole", "mppi", [desc, desc])
    with pytest.raises(ValueError, match="not found in task registry"):
        make_spot_ensemble_controller("no_such_task", "mppi", [desc])


def test_the_older_makers_name_the_new_ones():
    from judo_amd.ensemble import check_task as ensemble_check
    from judo_amd.randomized import check_task as randomized_check

    t = _spot_task()
    with pytest.raises(ValueError, match=r"Spot policy.*make_spot_ensemble_controller"):
        ensemble_check(t)
    with pytest.raises(ValueError, match=r"Spot policy tasks have no randomised plan step.*make_spot_randomized_controller"):
        randomized_check(t)


def test_the_fleets_refuse_the_new_classes_by_their_mark():
    """Every fleet's `_check_member` begins with fleet.refuse_fr3_randomized, which refuses a member that carries the classes' mark."""
    from judo_amd.fleet import refuse_fr3_randomized
    from judo_amd.spot_plants import SpotEnsembleController, SpotRandomizedController

    for cls in (SpotEnsembleController, SpotRandomizedController):
        assert cls._spot_plants is True
        member = object.__new__(cls)  # (no device: the refusal reads the class alone)
        with pytest.raises(ValueError, match=rf"fleet member 1 is a {cls.__name__}.*plant 0 alone"):
            refuse_fr3_randomized(1, member, None)


def test_the_boundary_lists_the_new_symbols():
    from judo_amd import _lib

    header = open(os.path.join(ROOT, "include", "judo_amd.h")).read()
    declared = set(re.findall(r"\b(jh_[a-z_0-9]+)\s*\(", header))
    for name in NEW_SYMBOLS:
        assert name in _lib.EXPORTED_SYMBOLS and name in declared, name
    lib = _lib.lib()
    for name in NEW_SYMBOLS:
        assert getattr(lib, name).argtypes == _lib._SIGNATURES[name][1], name
