"""Randomised physics on the host: `models.scaled_description` perturbs masses, friction and gains, and the packed image moves in its float section alone -- the
invariant a model set (`jh_model_set_create`, `device.GpuModelSet`) rests on.  No GPU."""

import copy
import json

import numpy as np
import pytest

# (task, the perturbed members of tests/test_gpu_model_set.py: keyword arguments of scaled_description)
CASES = [
    ("cartpole", dict(body_mass={"pole": 1.5})),
    ("cartpole", dict(body_mass={"pole": 0.7}, actuator_kp={None: 1.2})),
    ("cylinder_push", dict(body_mass={"pusher": 1.5})),
    ("cylinder_push", dict(body_mass={"cart": 0.6}, actuator_kp={None: 1.2})),
    ("leap_cube", dict(body_mass={"cube": 1.5}, geom_friction={"cube": 0.6})),
    ("leap_cube", dict(actuator_kp={None: 1.2})),
    ("leap_cube", dict(body_mass={"cube": 0.7}, geom_friction={"cube": 1.3}, actuator_kp={None: 0.85})),
    ("leap_cube_down", dict(body_mass={"cube": 1.5}, geom_friction={"cube": 0.6})),
    ("caltech_leap_cube", dict(body_mass={"cube": 1.5}, geom_friction={"cube": 0.6})),
]


def _task_desc(task):
    from judo_amd.tasks import get_registered_tasks

    return get_registered_tasks()[task][0]().desc


@pytest.mark.parametrize("task,kw", CASES, ids=[f"{t}-{i}" for i, (t, _) in enumerate(CASES)])
def test_scaled_description_moves_the_float_section_alone(task, kw):
    from judo_amd.models import image_sections, pack_model, scaled_description

    desc = _task_desc(task)
    before = json.dumps(desc, sort_keys=True)
    scaled = scaled_description(desc, **kw)
    assert json.dumps(desc, sort_keys=True) == before, "the input description was mutated"
    base, pert = pack_model(desc), pack_model(scaled)
    assert len(base) == len(pert)
    (h0, f0, i0), (h1, f1, i1) = image_sections(base), image_sections(pert)
    assert h0 == h1 and len(h0) == 64
    assert i0 == i1
    assert len(f0) == len(f1) and f0 != f1
    assert h0 + f0 + i0 == base
    changed = int((np.frombuffer(f0, np.uint32) != np.frombuffer(f1, np.uint32)).sum())
    assert 1 <= changed <= 400  # (a handful of words: masses, inertias, inverse weights, friction, gains -- 2-4 for the closed-form models, some hundreds at most for the leap family)


def test_scaled_description_scales_what_it_names_and_nothing_else():
    from judo_amd.models import scaled_description

    desc = _task_desc("leap_cube")
    s = scaled_description(desc, body_mass={"cube": 1.5}, geom_friction={"cube": 0.6}, actuator_kp={None: 1.2, "if_mcp_act": 0.5})
    cube0, cube1 = (next(b for b in d["bodies"] if b["name"] == "cube") for d in (desc, s))
    assert cube1["mass"] == cube0["mass"] * 1.5 and cube1["inertia"] == [v * 1.5 for v in cube0["inertia"]]
    g0, g1 = (next(g for g in d["geoms"] if g["name"] == "cube") for d in (desc, s))
    assert g1["friction"] == [g0["friction"][0] * 0.6] + g0["friction"][1:]
    for a0, a1 in zip(desc["actuators"], s["actuators"]):
        assert a1["kp"] == a0["kp"] * 1.2 * (0.5 if a0["name"] == "if_mcp_act" else 1.0)
    # everything that was not named is equal
    t = copy.deepcopy(s)
    next(b for b in t["bodies"] if b["name"] == "cube").update(mass=cube0["mass"], inertia=cube0["inertia"])
    next(g for g in t["geoms"] if g["name"] == "cube").update(friction=g0["friction"])
    for a0, a1 in zip(desc["actuators"], t["actuators"]):
        a1["kp"] = a0["kp"]
    assert t == desc
    assert scaled_description(desc) == desc and scaled_description(desc) is not desc


@pytest.mark.parametrize("kw", [dict(body_mass={"no_such_body": 2.0}), dict(geom_friction={"no_such_geom": 2.0}), dict(actuator_kp={"no_such_actuator": 2.0})])
def test_scaled_description_refuses_unknown_names(kw):
    from judo_amd.models import scaled_description

    with pytest.raises(ValueError, match="no_such"):
        scaled_description(_task_desc("cartpole"), **kw)


def test_a_structural_edit_moves_the_int_section():
    """What the fleet's check and jh_model_set_create refuse: a description edited in its topology packs to another int section -- with another <exclude> pair (palm /
    if_bs collide, if_px / mf_px do not) the header and the float section stay and the pair lists move; with one pair less the int section grows."""
    from judo_amd.models import image_sections, pack_model

    desc = _task_desc("leap_cube")
    edited = copy.deepcopy(desc)
    edited["excludes"][0] = [6, 10]
    (h0, f0, i0), (h1, f1, i1) = image_sections(pack_model(desc)), image_sections(pack_model(edited))
    assert h0 == h1 and f0 == f1 and len(i0) == len(i1) and i0 != i1
    edited["excludes"] = desc["excludes"][1:]
    h2, _, i2 = image_sections(pack_model(edited))
    assert h2 != h0 and len(i2) > len(i0)


def test_image_sections_refuses_what_is_no_image():
    from judo_amd.models import image_sections, pack_model

    blob = pack_model(_task_desc("cartpole"))
    with pytest.raises(ValueError):
        image_sections(blob[:-4])
    with pytest.raises(ValueError):
        image_sections(b"\0" * 64)
