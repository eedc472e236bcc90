"""The host side of the randomised fleet, without a device: the limits of a launch, the weights in the shared and the per-member form with the largest-remainder
assignment per member, the refusals that come before any model is made, and the new entry in the header and the ctypes shim."""

import copy
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _descs(task, perturbations):
    from judo_amd.models import scaled_description
    from judo_amd.tasks import get_registered_tasks

    desc = get_registered_tasks()[task][0]().desc
    return [copy.deepcopy(desc)] + [scaled_description(desc, **kw) for kw in perturbations]


def test_the_constant_and_the_entry_agree_with_the_header():
    from judo_amd import _lib
    from judo_amd.randomized_fleet import MAX_FLEET_PLANT_BLOCKS

    header = open(os.path.join(ROOT, "include", "judo_amd.h")).read()
    m = re.search(r"#define\s+JH_MAX_FLEET_PLANT_BLOCKS\s+(\d+)", header)
    assert m and int(m.group(1)) == _lib.MAX_FLEET_PLANT_BLOCKS == MAX_FLEET_PLANT_BLOCKS
    assert MAX_FLEET_PLANT_BLOCKS % 4 == 0 and MAX_FLEET_PLANT_BLOCKS >= _lib.MAX_PLANT_BLOCKS  # (four entries to a word; one controller's G always fits)
    m = re.search(r"\bint\s+jh_plan_step_randomized_batch\s*\(([^;]*)\);", header)
    assert m, "include/judo_amd.h does not declare jh_plan_step_randomized_batch"
    params = [p.strip() for p in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",")]
    restype, argtypes = _lib._SIGNATURES["jh_plan_step_randomized_batch"]
    assert len(params) == len(argtypes) == 31 and "jh_plan_step_randomized_batch" in _lib.EXPORTED_SYMBOLS
    assert params[1] == "int B" and params[2] == "int M" and params[18].replace(" ", "") == "constunsignedchar*plant_of_block" and params[19] == "int G"
    # the order of jh_plan_step_ensemble_batch, with the tables and G where that call has member_costs, costs and worst
    ens = re.search(r"\bint\s+jh_plan_step_ensemble_batch\s*\(([^;]*)\);", header)
    ens = [p.strip() for p in re.sub(r"/\*.*?\*/", "", ens.group(1), flags=re.S).split(",")]
    assert params[:18] == ens[:18] and params[21:] == ens[21:] and params[20] == ens[19]


def test_the_limits_of_a_launch():
    from judo_amd import _lib
    from judo_amd.randomized_fleet import check_fleet_blocks

    limit = _lib.MAX_FLEET_PLANT_BLOCKS
    check_fleet_blocks(1, 1)
    check_fleet_blocks(limit // 64, 64)
    check_fleet_blocks(_lib.MAX_ENSEMBLE_FLEET, limit // _lib.MAX_ENSEMBLE_FLEET)
    with pytest.raises(ValueError, match="at least one controller"):
        check_fleet_blocks(0, 4)
    with pytest.raises(ValueError, match="257.*JH_MAX_ENSEMBLE_FLEET"):
        check_fleet_blocks(257, 1)
    with pytest.raises(ValueError, match="65 blocks.*JH_MAX_PLANT_BLOCKS"):
        check_fleet_blocks(2, 65)
    with pytest.raises(ValueError, match="0 blocks"):
        check_fleet_blocks(2, 0)
    B = limit // 64 + 1
    with pytest.raises(ValueError, match=rf"B \* G = {B} \* 64 = {B * 64} .*exceed the {limit} .*JH_MAX_FLEET_PLANT_BLOCKS"):
        check_fleet_blocks(B, 64)


def test_weights_in_both_forms():
    from judo_amd.randomized_fleet import fleet_weights

    assert fleet_weights(3, 2, None) == [None, None, None]
    assert fleet_weights(3, 2, [1, 3]) == [[1.0, 3.0]] * 3
    assert fleet_weights(2, 3, [[1, 0, 0], (0, 2, 2)]) == [[1.0, 0.0, 0.0], [0.0, 2.0, 2.0]]
    assert fleet_weights(2, 2, [[1, 1], [0, 1]]) == [[1.0, 1.0], [0.0, 1.0]]  # (B == M: two lists are two members' weights)
    with pytest.raises(ValueError, match="3 weights for M = 2"):
        fleet_weights(3, 2, [1, 1, 1])
    with pytest.raises(ValueError, match="mixture"):
        fleet_weights(2, 2, [[1, 1], 1])
    with pytest.raises(ValueError, match="3 lists of weights for a fleet of 2"):
        fleet_weights(2, 2, [[1, 1], [1, 1], [1, 1]])
    with pytest.raises(ValueError, match="fleet member 1: 3 weights for M = 2"):
        fleet_weights(2, 2, [[1, 1], [1, 1, 1]])


def test_largest_remainder_per_member():
    from judo_amd.randomized_fleet import fleet_assignments

    assert fleet_assignments(2, 3, 3, None) == [[0, 1, 2], [0, 1, 2]]
    assert fleet_assignments(2, 3, 5, None) == [[0, 1, 2, 0, 1]] * 2  # (no weights: block g on plant g % M)
    assert fleet_assignments(2, 3, 8, [0.7, 0.2, 0.1]) == [[0, 0, 0, 0, 0, 0, 1, 2]] * 2  # quotas 5.6, 1.6, 0.8: floor 5 1 0, the open blocks to 0.8 and to the lower of the tied 0.6
    got = fleet_assignments(3, 3, 4, [[1, 1, 1], [1, 0, 0], [0, 1, 3]])
    assert got == [[0, 0, 1, 2], [0, 0, 0, 0], [1, 2, 2, 2]]
    with pytest.raises(ValueError, match=r"fleet member 1: weights must be non-negative"):
        fleet_assignments(2, 2, 4, [[1, 1], [0, 0]])
    with pytest.raises(ValueError, match="JH_MAX_FLEET_PLANT_BLOCKS"):
        fleet_assignments(200, 2, 64, None)


def test_the_other_fleets_name_the_randomized_fleet():
    """`ControllerFleet` and `EnsembleFleet` refuse a randomised member before they touch a device; the texts still name its call, and now the fleet that takes it."""
    from judo_amd.ensemble_fleet import EnsembleFleet
    from judo_amd.fleet import ControllerFleet
    from judo_amd.randomized import RandomizedController
    from judo_amd.randomized_fleet import RandomizedFleet

    c = RandomizedController.__new__(RandomizedController)  # (no model, no device: the refusal looks at the type alone)
    c.device = None
    for fleet in (ControllerFleet, EnsembleFleet):
        with pytest.raises(ValueError, match=r"fleet member 0 is a RandomizedController.*jh_plan_step_randomized.*RandomizedFleet.*make_randomized_fleet"):
            fleet([c])
    assert RandomizedFleet._randomized_members and not ControllerFleet._randomized_members and not EnsembleFleet._randomized_members

    class Plain:
        device = None

    with pytest.raises(ValueError, match="fleet member 0 is a Plain, not a RandomizedController"):
        RandomizedFleet([Plain()])


def test_fr3_and_spot_are_refused_without_a_device():
    """With the single controller's messages, before anything is packed or made."""
    from judo_amd.randomized_fleet import make_randomized_fleet
    from judo_amd.tasks import get_registered_tasks

    tasks = get_registered_tasks()
    with pytest.raises(ValueError, match="fr3_pick has no randomised plan step"):
        make_randomized_fleet("fr3_pick", "cem", 2, [tasks["fr3_pick"][0]().desc])
    with pytest.raises(ValueError, match="Spot policy tasks have no randomised plan step"):
        make_randomized_fleet("spot_box_push", "mppi", 2, [tasks["spot_box_push"][0]().desc])
    with pytest.raises(ValueError, match="not found in task registry"):
        make_randomized_fleet("no_such_task", "mppi", 2, [])
    cart = _descs("cartpole", [dict(body_mass={"pole": 1.5})])
    with pytest.raises(ValueError, match=r"fleet member 1 differs from member 0 in the number of plants M: 1 against 2"):
        make_randomized_fleet("cartpole", "mppi", 2, [cart, cart[:1]])
    with pytest.raises(ValueError, match="JH_MAX_FLEET_PLANT_BLOCKS"):
        make_randomized_fleet("cartpole", "mppi", 200, cart, blocks=64)
