"""The host side of the fr3_pick fleet (no GPU): the header, the ctypes table and the built library agree on jh_plan_step_batch_phases, and the module imports."""

import ctypes
import os
import re

from tests.conftest import ROOT


def _prototype(header: str, name: str) -> list[str]:
    """The parameter names of `name`'s prototype in the header, in order."""
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", header)
    assert m, f"{name} is not declared"
    params = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",")
    return [re.findall(r"[A-Za-z_0-9]+", p)[-1] for p in params]


def test_header_declares_the_phases_entry_with_o_phase_behind_o_lohi():
    header = open(os.path.join(ROOT, "include", "judo_amd.h")).read()
    base, phases = _prototype(header, "jh_plan_step_batch"), _prototype(header, "jh_plan_step_batch_phases")
    i = base.index("o_lohi")
    assert phases == base[: i + 1] + ["o_phase"] + base[i + 1 :]


def test_ctypes_row_matches_and_the_library_exports_the_symbol():
    from judo_amd import _lib

    res_b, args_b = _lib._SIGNATURES["jh_plan_step_batch"]
    res_p, args_p = _lib._SIGNATURES["jh_plan_step_batch_phases"]
    i = 10  # m, B, blk_dev, blk_host, blk_bytes, blk_stride_bytes, o_nominal, o_sigma, o_tp, o_lohi
    assert res_p is res_b is ctypes.c_int
    assert args_p == args_b[:i] + [ctypes.c_int] + args_b[i:]
    assert "jh_plan_step_batch_phases" in _lib.EXPORTED_SYMBOLS
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "jh_plan_step_batch_phases")


def test_fr3_fleet_imports_without_a_device():
    from judo_amd import fr3_fleet
    from judo_amd.fleet import ControllerFleet

    assert issubclass(fr3_fleet.FR3Fleet, ControllerFleet) and callable(fr3_fleet.make_fr3_fleet)
    assert fr3_fleet.FR3Fleet._block_extra_words == 1 and ControllerFleet._block_extra_words == 0
