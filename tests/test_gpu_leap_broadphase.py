"""The lane mapping of the hand's broad phase (jh_engine_v5.hip: the list-driven level 1 and the combination-per-lane level 2) changes where a test runs and nothing else: the candidate list of every
rollout and step keeps its entries and their order, so every output keeps its bits.  Compared word for word with tests/golden/leap_broadphase_bits.npz, the kernel's own
output from before the mapping was changed (tools/record_leap_broadphase_bits.py, which is also this test's runner; the fixture's metadata names the commit and compiler):
tangled hand configurations chosen so that the recorded rollout-steps have more than 16 box survivors at level 1, a body pair with more than 16 geom combinations and pairs with
one near geom on either side, with no contact dropped (a step without any sphere survivor was looked for and not found) -- on the 48-contact build, the 64-contact build (leap_cube_down), caltech_leap_cube
(122 body pairs: a ragged last pass of level 1) with spheres and with cylinders at the fingertips, and in the latency mode (rows of a wave computing copies).  No tolerance
appears in this file."""

import importlib.util
import json
import os

import numpy as np
import pytest

from tests.conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu

_spec = importlib.util.spec_from_file_location("record_leap_broadphase_bits", os.path.join(ROOT, "tools", "record_leap_broadphase_bits.py"))
rec = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(rec)


@pytest.fixture(scope="module")
def golden():
    d = np.load(os.path.join(GOLDEN, "leap_broadphase_bits.npz"))
    return d, json.loads(bytes(d["meta"]).decode())


def _same_words(what, got, want):
    got, want = np.ascontiguousarray(got).view(np.uint32), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    diff = int((got != want).sum())
    print(f"{what}: {diff} of {want.size} words differ")
    assert diff == 0, (what, diff, want.size)


def test_the_fixture_covers_the_loops(golden):
    """Conditions on the recorded rollout-steps, checked with the kernel's diagnostic counters when the fixture was recorded."""
    d, meta = golden
    assert set(meta["cases"]) == set(rec.CASES) and meta["H"] == rec.H and tuple(meta["counters"]) == rec.COUNTERS
    # "step_without_sphere_survivor" is recorded in the metadata and not asserted: no hand configuration produced one (never fewer than 8 survivors in 12.6 million rollout-steps
    # of the headline workload and among the recorder's candidates, clenched and spread fingers and arbitrary joint angles included; profiles/leap_broad_phase.md section 5)
    for cond in ("box_survivors_above_16", "combinations_above_16", "one_near_geom_A", "one_near_geom_B"):
        assert meta["coverage"][cond], cond
    assert set(meta["coverage"]) == set(rec.CONDITIONS)
    for name, m in meta["cases"].items():
        assert m["materialize_counters"][0] == 0 and m["cost_counters"][0] == 0, name  # no contact dropped: the comparison does not test the drop rule
        assert d[f"{name}/x0"].shape == (rec.CASES[name]["N"], 45) and np.isfinite(d[f"{name}/x0"]).all()


@pytest.mark.parametrize("name", list(rec.CASES))
def test_materialized_rollouts_keep_their_bits(gpu, golden, name):
    """jh_rollout_materialize: states, sensors and the solver counters."""
    d, _ = golden
    case = rec.CASES[name]
    s, y, c = rec.run_materialize(rec.gpu_model(case), d[f"{name}/x0"], d[f"{name}/U"], case["shift"])
    assert s.shape == (case["N"], rec.H, 45)
    _same_words(f"{name} states", s, d[f"{name}/states"])
    _same_words(f"{name} sensors", y, d[f"{name}/sensors"])
    assert c.tolist() == d[f"{name}/materialize_counters"].tolist(), (name, dict(zip(rec.COUNTERS, c.tolist())), d[f"{name}/materialize_counters"].tolist())


@pytest.mark.parametrize("name", list(rec.CASES))
def test_fused_rollout_costs_keep_their_bits(gpu, golden, name):
    """jh_rollout_cost_traced from a tangled start state: costs, trace rows and the solver counters."""
    d, meta = golden
    case = rec.CASES[name]
    blk = {k: d[f"{name}/blk_{k}"] for k in ("x0", "nominal", "sigma", "lohi", "tp", "W")}
    blk["phase"] = meta["cases"][name]["phase"]
    costs, trace, c = rec.run_cost_traced(rec.gpu_model(case), blk, d[f"{name}/noise"], case["N"], case["shift"])
    _same_words(f"{name} costs", costs, d[f"{name}/costs"])
    _same_words(f"{name} trace", trace, d[f"{name}/trace"])
    assert c.tolist() == d[f"{name}/cost_counters"].tolist(), (name, dict(zip(rec.COUNTERS, c.tolist())), d[f"{name}/cost_counters"].tolist())
