"""The host side of the ensemble fleet, without a device: the admission rule on descriptions in the shared and the per-member form, the `worst` normalisation, and the new
entry in the header and the ctypes shim."""

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


def test_descriptions_in_both_forms():
    from judo_amd.ensemble_fleet import check_fleet_descriptions, fleet_descriptions

    shared = _descs("cartpole", [dict(body_mass={"pole": 1.5}), dict(body_mass={"pole": 0.7})])
    lists = fleet_descriptions(4, shared)
    assert len(lists) == 4 and all(len(ds) == 3 and all(a is b for a, b in zip(ds, shared)) for ds in lists)
    blobs = check_fleet_descriptions(lists)
    assert len(blobs) == 4 and all(len(b) == 3 for b in blobs) and blobs[1][2] == blobs[0][2] and blobs[0][1] != blobs[0][0]

    own = [_descs("cartpole", [dict(body_mass={"pole": 1.5})]), _descs("cartpole", [dict(actuator_kp={None: 1.2})])]
    own[1][0] = _descs("cartpole", [dict(body_mass={"cart": 1.1})])[1]  # (member 1's plant 0 is not the shipped model either)
    lists = fleet_descriptions(2, own)
    assert [len(ds) for ds in lists] == [2, 2] and lists[1][1] is own[1][1]
    blobs = check_fleet_descriptions(lists)
    assert blobs[1][0] != blobs[0][0]

    with pytest.raises(ValueError, match="3 lists of descriptions for a fleet of 2"):
        fleet_descriptions(2, [shared, shared, shared])
    with pytest.raises(ValueError, match="mixture"):
        fleet_descriptions(2, [shared, shared[0]])
    with pytest.raises(ValueError, match="at least one controller"):
        fleet_descriptions(0, shared)
    with pytest.raises(ValueError, match="257.*JH_MAX_ENSEMBLE_FLEET"):
        fleet_descriptions(257, shared)
    with pytest.raises(ValueError, match="at least one description"):
        fleet_descriptions(2, [])


def test_admission_rule_names_the_member_and_the_field():
    from judo_amd.ensemble_fleet import check_fleet_descriptions

    cart = _descs("cartpole", [dict(body_mass={"pole": 1.5})])
    with pytest.raises(ValueError, match=r"fleet member 1 differs from member 0 in the number of plants M: 1 against 2"):
        check_fleet_descriptions([cart, cart[:1]])
    cyl = _descs("cylinder_push", [dict(body_mass={"pusher": 1.5})])
    with pytest.raises(ValueError, match=r"fleet member 2 has another model image than member 0: the (header|float section|int section)"):
        check_fleet_descriptions([cart, cart, cyl])
    with pytest.raises(ValueError, match=r"fleet member 1: ensemble member 1 has another model image than member 0"):
        check_fleet_descriptions([cart, [cart[0], cyl[0]]])
    with pytest.raises(ValueError, match="fleet member 0: an ensemble needs at least one description"):
        check_fleet_descriptions([[], cart])


def test_worst_normalisation():
    from judo_amd.ensemble_fleet import fleet_worst

    assert fleet_worst(3, 4, None) == [4, 4, 4]  # the mean
    assert fleet_worst(3, 4, 2) == [2, 2, 2]
    assert fleet_worst(3, 4, [1, 2, 4]) == [1, 2, 4] and fleet_worst(2, 4, (3, 1)) == [3, 1]
    with pytest.raises(ValueError, match="2 values of worst for a fleet of 3"):
        fleet_worst(3, 4, [1, 2])
    with pytest.raises(ValueError, match=r"fleet member 1: worst = 5 outside \[1, M = 4\]"):
        fleet_worst(3, 4, [1, 5, 2])
    with pytest.raises(ValueError, match=r"fleet member 0: worst = 0"):
        fleet_worst(2, 4, 0)


def test_the_entry_is_declared_and_bound():
    from judo_amd import _lib

    header = open(os.path.join(ROOT, "include", "judo_amd.h")).read()
    m = re.search(r"\bint\s+jh_plan_step_ensemble_batch\s*\(([^;]*)\);", header)
    assert m, "include/judo_amd.h does not declare jh_plan_step_ensemble_batch"
    params = [p.strip() for p in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",")]
    restype, argtypes = _lib._SIGNATURES["jh_plan_step_ensemble_batch"]
    assert len(params) == len(argtypes) == 31 and "jh_plan_step_ensemble_batch" in _lib.EXPORTED_SYMBOLS
    assert params[1] == "int B" and params[2] == "int M" and params[20].replace(" ", "") == "constint*worst"
    m = re.search(r"#define\s+JH_MAX_ENSEMBLE_FLEET\s+(\d+)", header)
    assert m and int(m.group(1)) == _lib.MAX_ENSEMBLE_FLEET == 256
