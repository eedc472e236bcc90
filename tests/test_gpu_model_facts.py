"""What the library answers about a model before anything is launched: the build it selects, its limits, its trace layout, the knot bounds of the fused and of the
one-launch plan step, and whether a one-launch plan step can be forced -- for every shipped image, at both contact capacities of the leap family and at the cross-check
kernel generations where `jh_model_set_kernel` takes them.  Handles only: no kernel runs.

These answers come from the build table (`jh_engine_build`, judo_amd/csrc/jh_internal.h) and the few lines of `jh_api.hip` around it.  The literals in EXPECTED were
recorded by running `facts()` below, this file's own test body, against the library built from commit ff0640b -- the last one that answered them with chains of
comparisons on the model kind -- selected with JUDO_AMD_LIB, and this file passes on that library unchanged.  They are not taken from the code they now test."""

import ctypes as C
import functools

import pytest

from judo_amd import _lib
from judo_amd.models import load_description, pack_model

pytestmark = pytest.mark.gpu

HORIZONS = (1, 16, 64, 250, 1000)
# model -> the description it is packed from
MODELS = {
    "cartpole": lambda: load_description("cartpole"),
    "cylinder_push": lambda: load_description("cylinder_push"),
    "leap_cube": lambda: load_description("leap_cube"),
    "leap_cube_down": lambda: load_description("leap_cube_down"),
    "caltech_leap_cube": lambda: load_description("caltech_leap_cube"),
    "caltech_leap_cube_cylinder": lambda: dict(load_description("caltech_leap_cube"), fingertips="cylinder"),
    "fr3_pick": lambda: load_description("fr3_pick"),
    "fr3_pick_self": lambda: dict(load_description("fr3_pick"), self_collision=True),
}
LEAP = ("leap_cube", "leap_cube_down", "caltech_leap_cube", "caltech_leap_cube_cylinder")
# (model, contact capacity asked for or None, kernel generation): the leap family at 48 and 64 contacts; every model at generations 2 and 1 as well (the closed-form
# models take the setting without effect, the cylinder and self-collision images refuse it)
CASES = [(name, cap, gen) for name in MODELS for cap in ((48, 64) if name in LEAP else (None,)) for gen in (3, 2, 1)]


@functools.lru_cache(maxsize=None)
def blob(name: str) -> bytes:
    return pack_model(MODELS[name]())  # (half a second for a leap image: packed once per model, a handle per case)


def case_id(case) -> str:
    name, cap, gen = case
    return name + (f"-cap{cap}" if cap else "") + f"-gen{gen}"


def facts(case) -> dict:
    """Everything the library says about the model of `case` through its query entries, as plain ints and strings.  A setter that refuses is part of the answer: its
    status and message are recorded and the model is asked as it stands."""
    name, cap, gen = case
    L = _lib.lib()
    m = C.c_void_p()
    _lib.check(L.jh_model_create(C.create_string_buffer(blob(name), len(blob(name))), len(blob(name)), 0, C.byref(m)), "jh_model_create")

    def said(status: int) -> list:
        return [int(status), L.jh_last_error().decode() if status else ""]

    def ints(fn, n: int) -> list:
        out = (C.c_int * n)()
        assert fn(m, out) == 0
        return [int(v) for v in out]

    f = {}
    if cap is not None:
        f["set_contact_capacity"] = said(L.jh_model_set_contact_capacity(m, cap))
    if gen != 3:
        f["set_kernel"] = said(L.jh_model_set_kernel(m, gen))
    f["build"] = ints(L.jh_model_build, 4)
    f["fr3_build"] = ints(L.jh_model_fr3_build, 4)
    f["limits"] = ints(L.jh_model_limits, 4)
    f["trace_layout"] = ints(L.jh_model_trace_layout, 3)
    f["max_fused_knots"] = [int(L.jh_model_max_fused_knots(m, H)) for H in HORIZONS]
    f["one_launch_max_knots"] = [int(L.jh_model_one_launch_max_knots(m, H)) for H in HORIZONS]
    f["force_one_launch"] = said(L.jh_model_set_plan_step_launches(m, 1))
    L.jh_model_destroy(m)
    return f


# the refusals, word for word
CYL_64 = "model_set_contact_capacity: the cylinder build of the leap kernel holds 64 contacts per rollout (got 48)"
GEN3_ARM_PAIRS = "model_set_kernel: the image holds 112 pairs between arm bodies; only generation 3 (the self-collision build of the fr3 kernel) collides them"
GEN3_CYLINDERS = "model_set_kernel: the image holds 4 cylinder geoms; only generation 3 (the cylinder build of the leap kernel) collides them"
TWO_LAUNCHES = "model_set_plan_step_launches: only the closed-form models have a one-launch plan step"
EXPECTED = {
    "cartpole-gen3": {"build": [2, 0, 0, 0], "fr3_build": [0, 0, 0, 0], "limits": [251, 512, 32, 0], "trace_layout": [0, 6, 1], "max_fused_knots": [251, 204, 127, 52, 15], "one_launch_max_knots": [47, 45, 38, 24, 9], "force_one_launch": [0, ""]},
    "cartpole-gen2": {"set_kernel": [0, ""], "build": [2, 0, 0, 0], "fr3_build": [0, 0, 0, 0], "limits": [251, 512, 32, 0], "trace_layout": [0, 6, 1], "max_fused_knots": [251, 204, 127, 52, 15], "one_launch_max_knots": [47, 45, 38, 24, 9], "force_one_launch": [0, ""]},
    "cartpole-gen1": {"set_kernel": [0, ""], "build": [1, 0, 0, 0], "fr3_build": [0, 0, 0, 0], "limits": [251, 512, 32, 0], "trace_layout": [0, 6, 1], "max_fused_knots": [251, 204, 127, 52, 15], "one_launch_max_knots": [47, 45, 38, 24, 9], "force_one_launch": [0, ""]},
    "cylinder_push-gen3": {"build": [2, 0, 0, 0], "fr3_build": [0, 0, 0, 0], "limits": [126, 512, 32, 0], "trace_layout": [0, 6, 1], "max_fused_knots": [126, 113, 85, 43, 14], "one_launch_max_knots": [23, 23, 21, 16, 8], "force_one_launch": [0, ""]},
    "cylinder_push-gen2": {"set_kernel": [0, ""], "build": [2, 0, 0, 0], "fr3_build": [0, 0, 0, 0], "limits": [126, 512, 32, 0], "trace_layout": [0, 6, 1], "max_fused_knots": [126, 113, 85, 43, 14], "one_launch_max_knots": [23, 23, 21, 16, 8], "force_one_launch": [0, ""]},
    "cylinder_push-gen1": {"set_kernel": [0, ""], "build": [1, 0, 0, 0], "fr3_build": [0, 0, 0, 0], "limits": [126, 512, 32, 0], "trace_layout": [0, 6, 1], "max_fused_knots": [126, 113, 85, 43, 14], "one_launch_max_knots": [23, 23, 21, 16, 8], "force_one_launch": [0, ""]},
    "leap_cube-cap48-gen3": {"set_contact_capacity": [0, ""], "build": [3, 48, 0, 0], "fr3_build": [0, 0, 0, 0], "limits": [32, 512, 32, 48], "trace_layout": [16, 15, 0], "max_fused_knots": [32, 32, 32, 32, 32], "one_launch_max_knots": [0, 0, 0, 0, 0], "force_one_launch": [-1, TWO_LAUNCHES]},
    "leap_cube-cap48-gen2": {"set_contact_capacity": [0, ""], "set_kernel": [0, ""], "build": [2, 0, 0, 0], "fr3_build": [0, 0, 0, 0], "limits": [8, 512, 32, 32], "trace_layout": [0, 0, 0], "max_fused_knots": [8, 8, 8, 8, 8], "one_launch_max_knots": [0, 0, 0, 0, 0], "force_one_launch": [-1, TWO_LAUNCHES]},
    "leap_cube-cap48-gen1": {"set_contact_capacity": [0, ""], "set_kernel": [0, ""], "build": [1, 0, 0, 0], "fr3_build": [0, 0, 0, 0], "limits": [9, 512, 32, 32], "trace_layout": [0, 0, 0], "max_fused_knots": [9, 9, 9, 7, 5], "one_launch_max_knots": [0, 0, 0, 0, 0], "force_one_launch": [-1, TWO_LAUNCHES]},
    "leap_cube-cap64-gen3": {"set_contact_capacity": [0, ""], "build": [3, 64, 0, 0], "fr3_build": [0, 0, 0, 0], "limits": [32, 512, 32, 64], "trace_layout": [16, 15, 0], "max_fused_knots": [32, 32, 32, 32, 32], "one_launch_max_knots": [0, 0, 0, 0, 0], "force_one_launch": [-1, TWO_LAUNCHES]},
    "leap_cube-cap64-gen2": {"set_contact_capacity": [0, ""], "set_kernel": [0, ""], "build": [2, 0, 0, 0], "fr3_build": [0, 0, 0, 0], "limits": [8, 512, 32, 32], "trace_layout": [0, 0, 0], "max_fused_knots": [8, 8, 8, 8, 8], "one_launch_max_knots": [0, 0, 0, 0, 0], "force_one_launch": [-1, TWO_LAUNCHES]},
    "leap_cube-cap64-gen1": {"set_contact_capacity": [0, ""], "set_kernel": [0, ""], "build": [1, 0, 0, 0], "fr3_build": [0, 0, 0, 0], "limits": [9, 512, 32, 32], "trace_layout": [0, 0, 0], "max_fused_knots": [9, 9, 9, 7, 5], "one_launch_max_knots": [0, 0, 0, 0, 0], "force_one_launch": [-1, TWO_LAUNCHES]},
    "leap_cube_down-cap48-gen3": {"set_contact_capacity": [0, ""], "build": [3, 48, 0, 0], "fr3_build": [0, 0, 0, 0], "limits": [32, 512, 32, 48], "trace_layout": [16, 15, 0], "max_fused_knots": [32, 32, 32, 32, 32], "one_launch_max_knots": [0, 0, 0, 0, 0], "force_one_launch": [-1, TWO_LAUNCHES]},
    "leap_cube_down-cap48-gen2": {"set_contact_capacity": [0, ""], "set_kernel": [0, ""], "build": [2, 0, 0, 0], "fr3_build": [0, 0, 0, 0], "limits": [8, 512, 32, 32], "trace_layout": [0, 0, 0], "max_fused_knots": [8, 8, 8, 8, 8], "one_launch_max_knots": [0, 0, 0, 0, 0], "force_one_launch": [-1, TWO_LAUNCHES]},
    "leap_cube_down-cap48-gen1": {"set_contact_capacity": [0, ""], "set_kernel": [0, ""], "build": [1, 0, 0, 0], "fr3_build": [0, 0, 0, 0], "limits": [9, 512, 32, 32], "trace_layout": [0, 0, 0], "max_fused_knots": [9, 9, 9, 7, 5], "one_launch_max_knots": [0, 0, 0, 0, 0], "force_one_launch": [-1, TWO_LAUNCHES]},
    "leap_cube_down-cap64-gen3": {"set_contact_capacity": [0, ""], "build": [3, 64, 0, 0], "fr3_build": [0, 0, 0, 0], "limits": [32, 512, 32, 64], "trace_layout": [16, 15, 0], "max_fused_knots": [32, 32, 32, 32, 32], "one_launch_max_knots": [0, 0, 0, 0, 0], "force_one_launch": [-1, TWO_LAUNCHES]},
    "leap_cube_down-cap64-gen2": {"set_contact_capacity": [0, ""], "set_kernel": [0, ""], "build": [2, 0, 0, 0], "fr3_build": [0, 0, 0, 0], "limits": [8, 512, 32, 32], "trace_layout": [0, 0, 0], "max_fused_knots": [8, 8, 8, 8, 8], "one_launch_max_knots": [0, 0, 0, 0, 0], "force_one_launch": [-1, TWO_LAUNCHES]},
    "leap_cube_down-cap64-gen1": {"set_contact_capacity": [0, ""], "set_kernel": [0, ""], "build": [1, 0, 0, 0], "fr3_build": [0, 0, 0, 0], "limits": [9, 512, 32, 32], "trace_layout": [0, 0, 0], "max_fused_knots": [9, 9, 9, 7, 5], "one_launch_max_knots": [0, 0, 0, 0, 0], "force_one_launch": [-1, TWO_LAUNCHES]},
    "caltech_leap_cube-cap48-gen3": {"set_contact_capacity": [0, ""], "build": [3, 48, 0, 0], "fr3_build": [0, 0, 0, 0], "limits": [32, 512, 32, 48], "trace_layout": [0, 0, 0], "max_fused_knots": [32, 32, 32, 32, 32], "one_launch_max_knots": [0, 0, 0, 0, 0], "force_one_launch": [-1, TWO_LAUNCHES]},
    "caltech_leap_cube-cap48-gen2": {"set_contact_capacity": [0, ""], "set_kernel": [0, ""], "build": [2, 0, 0, 0], "fr3_build": [0, 0, 0, 0], "limits": [8, 512, 32, 32], "trace_layout": [0, 0, 0], "max_fused_knots": [8, 8, 8, 8, 8], "one_launch_max_knots": [0, 0, 0, 0, 0], "force_one_launch": [-1, TWO_LAUNCHES]},
    "caltech_leap_cube-cap48-gen1": {"set_contact_capacity": [0, ""], "set_kernel": [0, ""], "build": [1, 0, 0, 0], "fr3_build": [0, 0, 0, 0], "limits": [10, 512, 32, 32], "trace_layout": [0, 0, 0], "max_fused_knots": [10, 9, 9, 8, 5], "one_launch_max_knots": [0, 0, 0, 0, 0], "force_one_launch": [-1, TWO_LAUNCHES]},
    "caltech_leap_cube-cap64-gen3": {"set_contact_capacity": [0, ""], "build": [3, 64, 0, 0], "fr3_build": [0, 0, 0, 0], "limits": [32, 512, 32, 64], "trace_layout": [0, 0, 0], "max_fused_knots": [32, 32, 32, 32, 32], "one_launch_max_knots": [0, 0, 0, 0, 0], "force_one_launch": [-1, TWO_LAUNCHES]},
    "caltech_leap_cube-cap64-gen2": {"set_contact_capacity": [0, ""], "set_kernel": [0, ""], "build": [2, 0, 0, 0], "fr3_build": [0, 0, 0, 0], "limits": [8, 512, 32, 32], "trace_layout": [0, 0, 0], "max_fused_knots": [8, 8, 8, 8, 8], "one_launch_max_knots": [0, 0, 0, 0, 0], "force_one_launch": [-1, TWO_LAUNCHES]},
    "caltech_leap_cube-cap64-gen1": {"set_contact_capacity": [0, ""], "set_kernel": [0, ""], "build": [1, 0, 0, 0], "fr3_build": [0, 0, 0, 0], "limits": [10, 512, 32, 32], "trace_layout": [0, 0, 0], "max_fused_knots": [10, 9, 9, 8, 5], "one_launch_max_knots": [0, 0, 0, 0, 0], "force_one_launch": [-1, TWO_LAUNCHES]},
    "caltech_leap_cube_cylinder-cap48-gen3": {"set_contact_capacity": [-1, CYL_64], "build": [3, 64, 1, 4], "fr3_build": [0, 0, 0, 0], "limits": [32, 512, 32, 64], "trace_layout": [0, 0, 0], "max_fused_knots": [32, 32, 32, 32, 32], "one_launch_max_knots": [0, 0, 0, 0, 0], "force_one_launch": [-1, TWO_LAUNCHES]},
    "caltech_leap_cube_cylinder-cap48-gen2": {"set_contact_capacity": [-1, CYL_64], "set_kernel": [-3, GEN3_CYLINDERS], "build": [3, 64, 1, 4], "fr3_build": [0, 0, 0, 0], "limits": [32, 512, 32, 64], "trace_layout": [0, 0, 0], "max_fused_knots": [32, 32, 32, 32, 32], "one_launch_max_knots": [0, 0, 0, 0, 0], "force_one_launch": [-1, TWO_LAUNCHES]},
    "caltech_leap_cube_cylinder-cap48-gen1": {"set_contact_capacity": [-1, CYL_64], "set_kernel": [-3, GEN3_CYLINDERS], "build": [3, 64, 1, 4], "fr3_build": [0, 0, 0, 0], "limits": [32, 512, 32, 64], "trace_layout": [0, 0, 0], "max_fused_knots": [32, 32, 32, 32, 32], "one_launch_max_knots": [0, 0, 0, 0, 0], "force_one_launch": [-1, TWO_LAUNCHES]},
    "caltech_leap_cube_cylinder-cap64-gen3": {"set_contact_capacity": [0, ""], "build": [3, 64, 1, 4], "fr3_build": [0, 0, 0, 0], "limits": [32, 512, 32, 64], "trace_layout": [0, 0, 0], "max_fused_knots": [32, 32, 32, 32, 32], "one_launch_max_knots": [0, 0, 0, 0, 0], "force_one_launch": [-1, TWO_LAUNCHES]},
    "caltech_leap_cube_cylinder-cap64-gen2": {"set_contact_capacity": [0, ""], "set_kernel": [-3, GEN3_CYLINDERS], "build": [3, 64, 1, 4], "fr3_build": [0, 0, 0, 0], "limits": [32, 512, 32, 64], "trace_layout": [0, 0, 0], "max_fused_knots": [32, 32, 32, 32, 32], "one_launch_max_knots": [0, 0, 0, 0, 0], "force_one_launch": [-1, TWO_LAUNCHES]},
    "caltech_leap_cube_cylinder-cap64-gen1": {"set_contact_capacity": [0, ""], "set_kernel": [-3, GEN3_CYLINDERS], "build": [3, 64, 1, 4], "fr3_build": [0, 0, 0, 0], "limits": [32, 512, 32, 64], "trace_layout": [0, 0, 0], "max_fused_knots": [32, 32, 32, 32, 32], "one_launch_max_knots": [0, 0, 0, 0, 0], "force_one_launch": [-1, TWO_LAUNCHES]},
    "fr3_pick-gen3": {"build": [3, 0, 0, 0], "fr3_build": [0, 0, 1, 1], "limits": [8, 512, 32, 96], "trace_layout": [8, 6, 0], "max_fused_knots": [8, 8, 8, 8, 8], "one_launch_max_knots": [0, 0, 0, 0, 0], "force_one_launch": [-1, TWO_LAUNCHES]},
    "fr3_pick-gen2": {"set_kernel": [0, ""], "build": [2, 0, 0, 0], "fr3_build": [0, 0, 1, 1], "limits": [8, 512, 32, 32], "trace_layout": [0, 0, 0], "max_fused_knots": [8, 8, 8, 8, 8], "one_launch_max_knots": [0, 0, 0, 0, 0], "force_one_launch": [-1, TWO_LAUNCHES]},
    "fr3_pick-gen1": {"set_kernel": [0, ""], "build": [1, 0, 0, 0], "fr3_build": [0, 0, 1, 1], "limits": [27, 512, 32, 32], "trace_layout": [0, 0, 0], "max_fused_knots": [27, 26, 24, 18, 9], "one_launch_max_knots": [0, 0, 0, 0, 0], "force_one_launch": [-1, TWO_LAUNCHES]},
    "fr3_pick_self-gen3": {"build": [3, 0, 0, 0], "fr3_build": [1, 112, 0, 1], "limits": [8, 512, 32, 96], "trace_layout": [8, 6, 0], "max_fused_knots": [8, 8, 8, 8, 8], "one_launch_max_knots": [0, 0, 0, 0, 0], "force_one_launch": [-1, TWO_LAUNCHES]},
    "fr3_pick_self-gen2": {"set_kernel": [-3, GEN3_ARM_PAIRS], "build": [3, 0, 0, 0], "fr3_build": [1, 112, 0, 1], "limits": [8, 512, 32, 96], "trace_layout": [8, 6, 0], "max_fused_knots": [8, 8, 8, 8, 8], "one_launch_max_knots": [0, 0, 0, 0, 0], "force_one_launch": [-1, TWO_LAUNCHES]},
    "fr3_pick_self-gen1": {"set_kernel": [-3, GEN3_ARM_PAIRS], "build": [3, 0, 0, 0], "fr3_build": [1, 112, 0, 1], "limits": [8, 512, 32, 96], "trace_layout": [8, 6, 0], "max_fused_knots": [8, 8, 8, 8, 8], "one_launch_max_knots": [0, 0, 0, 0, 0], "force_one_launch": [-1, TWO_LAUNCHES]},
}


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_model_facts(gpu, case):
    assert facts(case) == EXPECTED[case_id(case)]
