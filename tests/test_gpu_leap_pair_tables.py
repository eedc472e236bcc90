"""The pair tables of the hand's broad phase (jh_engine_v5.hip level 1, judo_amd/engine_model.py::hand_pair_tables) take out body pairs that would have gone through level 2
and appended nothing: the same model packed with and without tables gives the same states, sensors, costs, trace rows and solver counters, word for word -- in materialise
mode and in the fused launch, on the three builds of the kernel and in the latency mode.  64 rollouts x 8 steps, knot noise 0.2.  The start states put safe and unsafe
rows side by side in every wave of four rollouts: the default pose; every finger's `pip` at -0.45 rad (inside its range, where the base link and the middle link do give a
candidate -- checked with the numpy restatement of tests/test_pair_tables.py); the table joints beyond the grid, anywhere on the circle; angles within 1e-6 rad of a
boundary between a safe and an unsafe cell.  No tolerance appears in this file."""

import copy
import functools
import importlib.util
import os

import numpy as np
import pytest

from tests.conftest import ROOT
from tests.test_pair_tables import Hand, finger_tables

pytestmark = pytest.mark.gpu

_spec = importlib.util.spec_from_file_location("record_leap_broadphase_bits", os.path.join(ROOT, "tools", "record_leap_broadphase_bits.py"))
rec = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(rec)

N, H, NOISE = 64, 8, 0.2
CASES = {name: dict(rec.CASES[name], N=N) for name in ("leap_cube", "leap_cube_down", "caltech_sphere", "caltech_cylinder")}
CASES["leap_cube_latency"] = dict(rec.CASES["leap_cube"], N=N, shift=None)  # (64 rollouts do not fill the GPU: the launcher lets rows of a wave compute copies)
KINDS = ("default", "pip_bent_back", "beyond_the_grid", "cell_boundary")


def _description(case):
    from judo_amd.models import load_description

    desc = load_description(case["task"])
    return dict(desc, fingertips="cylinder") if case["fingertips"] == "cylinder" else desc


@functools.lru_cache(maxsize=None)
def _pair(name):
    """(model with tables, model without, the image's tables and the fingers' three) of a case."""
    from judo_amd import engine_model as em
    from judo_amd.device import GpuModel

    case = CASES[name]
    desc = _description(case)
    with_t, without = GpuModel(copy.deepcopy(desc)), GpuModel(dict(copy.deepcopy(desc), pair_tables=False))
    tables = em.read_pair_tables(with_t._blob)
    assert len(tables) >= 3 and em.read_pair_tables(without._blob) == []
    for gm in (with_t, without):
        assert gm.build()["cylinder_build"] == (case["fingertips"] == "cylinder")
    fused = em.fuse_fixed_bodies(desc)
    st = em.engine_structure(fused)
    image = dict(blob=with_t._blob, tables=tables, code_name={i: fused["bodies"][b]["name"] for b, i in st["midx"].items()})
    return with_t, without, tables, finger_tables(image)


def _start_states(name):
    """(N, 45) start states, kind k in row n with n % 4 == k, so every wave of four rollouts holds all four kinds; and the kind of every row."""
    from judo_amd.tasks import get_registered_tasks

    case = CASES[name]
    gm, _, tables, fingers = _pair(name)
    assert sorted(fingers) == ["if", "mf", "rf"]
    from tests.test_gpu_model_set import _settled

    home = np.asarray(get_registered_tasks()[case["task"]][0]().default_state(), dtype=np.float64)
    # the cube where it rests in the hand after the oracle's settling steps (tests/test_gpu_model_set.py), so that the fingers' motion reaches the costs: from the home
    # state it is in free fall over eight steps whatever the hand does
    home[:7] = _settled(case["task"], 5 if case["task"] == "leap_cube_down" else 60)[:7]
    rng = np.random.default_rng(4242)
    xs = np.tile(home, (N, 1))
    xs[:, 23:] = 0.0
    kind = np.arange(N) % 4
    # 1: every finger's pip bent back to -0.45 rad: inside its range, in the strip where the pair does give a candidate
    for t in fingers.values():
        xs[kind == 1, 7 + t["j2"]] = -0.45
    hand = Hand(gm._blob, np.float32)
    for f, t in fingers.items():
        _, cand = hand.candidates(t["pair"], xs[kind == 1][:, 7:23].astype(np.float32))
        assert cand.all(), f"{name}: the {f} base and middle links give no candidate with pip at -0.45 rad: the start state does not exercise an unsafe cell"
    # 2: the table joints beyond the grid, anywhere on the circle
    rows = np.flatnonzero(kind == 2)
    for t in tables:
        for j, o, inv in ((t["j1"], t["o1"], t["inv1"]), (t["j2"], t["o2"], t["inv2"])):
            if inv == 0:
                continue
            lo, hi = o, o + 8.0 / inv
            below = rng.uniform(-np.pi, lo - 1e-3, len(rows))
            above = rng.uniform(hi + 1e-3, np.pi, len(rows))
            xs[rows, 7 + j] = np.where(rng.random(len(rows)) < 0.5, below, above)
    # 3: within 1e-6 rad of a boundary between a safe and an unsafe cell, on either side of it
    rows = np.flatnonzero(kind == 3)
    for t in tables:
        bit = lambda ix, iy: (t["word"] >> (ix + 8 * iy)) & 1  # noqa: E731
        edges = [(ix, iy) for ix in range(8) for iy in range(7) if bit(ix, iy) != bit(ix, iy + 1)] if t["inv2"] else []
        edges1 = [(ix, iy) for ix in range(7) for iy in range(8 if t["inv2"] else 1) if bit(ix, iy) != bit(ix + 1, iy)]
        assert edges or edges1, (name, t)
        for k, n in enumerate(rows):
            side = (-1e-6, 1e-6)[(k // 2) % 2]
            if edges and (k % 2 == 0 or not edges1):
                ix, iy = edges[(k // 4) % len(edges)]
                xs[n, 7 + t["j1"]] = t["o1"] + (ix + 0.5) / t["inv1"]
                xs[n, 7 + t["j2"]] = t["o2"] + (iy + 1) / t["inv2"] + side
            else:
                ix, iy = edges1[(k // 4) % len(edges1)]
                xs[n, 7 + t["j1"]] = t["o1"] + (ix + 1) / t["inv1"] + side
                if t["inv2"]:
                    xs[n, 7 + t["j2"]] = t["o2"] + (iy + 0.5) / t["inv2"]
    return xs.astype(np.float32), kind


def _same_words(what, a, b):
    a, b = np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    diff = int((a != b).sum())
    print(f"{what}: {diff} of {a.size} words differ")
    assert diff == 0, (what, diff, a.size)


@pytest.mark.parametrize("name", list(CASES))
def test_materialized_rollouts_are_the_same_with_and_without_tables(gpu, name):
    """jh_rollout_materialize from per-rollout start states: states, sensors and the solver counters."""
    from judo_amd import engine_model as em

    case = CASES[name]
    with_t, without, tables, _ = _pair(name)
    x0, kind = _start_states(name)
    # the rows differ in what the tables say at the start: safe and unsafe side by side in every wave
    safe = np.array([em.pair_table_safe(t, x0[:, 7 + t["j1"]], x0[:, 7 + t["j2"]]) for t in tables])
    assert safe[:, kind == 0].any() and not safe[:, kind == 2].any() and not safe.all(0)[kind == 1].any()
    assert len({tuple(c) for c in safe[:, kind == 3].T}) > 1, "the boundary rows fall on one side only"
    # ... and the table path has work to do: in the default rows and in some boundary rows a table reads safe for a pair that passes level 1 (bounding spheres and
    # boxes overlap), the pair the kernel takes off its list.  (The shipped library has no counter for it; profiles/leap_pair_tables.md has the COUNT build's.)
    hand = Hand(with_t._blob, np.float32)
    dropped = np.array([safe[i] & hand.candidates(t["pair"], x0[:, 7:23])[0] for i, t in enumerate(tables)])
    assert dropped[:, kind == 0].any(0).all() and dropped[:, kind == 3].any() and not dropped[:, kind == 2].any()
    rng = np.random.default_rng(99)
    U = (x0[:, None, 7:23] + NOISE * rng.standard_normal((N, H, 16))).astype(np.float32)
    sa, ya, ca = rec.run_materialize(with_t, x0, U, case["shift"])
    sb, yb, cb = rec.run_materialize(without, x0, U, case["shift"])
    assert sa.shape == (N, H, 45) and np.isfinite(sb).all() and np.isfinite(yb).all()
    _same_words(f"{name} states", sa, sb)
    _same_words(f"{name} sensors", ya, yb)
    assert ca.tolist() == cb.tolist(), (name, dict(zip(rec.COUNTERS, ca.tolist())), cb.tolist())
    assert cb[2] > 0 and cb[3] == N * H  # (Newton iterations were counted: the counters are live)


@functools.lru_cache(maxsize=None)
def _block(name):
    blk, K, nu = rec._plan_block({k: v for k, v in CASES[name].items()})
    return blk, K, nu


@pytest.mark.parametrize("name", list(CASES))
def test_fused_rollout_costs_are_the_same_with_and_without_tables(gpu, name):
    """jh_rollout_cost_traced from each kind of start state (a fused launch has one for all its rollouts; the knot noise spreads the rows): costs, trace rows, counters."""
    case = CASES[name]
    with_t, without, _, _ = _pair(name)
    x0, kind = _start_states(name)
    blk, K, nu = _block(name)
    blk = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in blk.items()}
    blk["sigma"] = np.full_like(blk["sigma"], NOISE)
    noise = np.random.default_rng(17).standard_normal((K, nu, N)).astype(np.float32)
    for k, what in enumerate(KINDS):
        row = x0[np.flatnonzero(kind == k)[k % 3]]
        blk["x0"] = row.reshape(blk["x0"].shape).copy()
        blk["nominal"] = np.tile(row[7:23], (K, 1)).reshape(blk["nominal"].shape).astype(np.float32)
        a = rec.run_cost_traced(with_t, blk, noise, N, case["shift"])
        b = rec.run_cost_traced(without, blk, noise, N, case["shift"])
        distinct = len(np.unique(np.concatenate([b[0].reshape(N, 1), b[1].reshape(N, -1)], axis=1), axis=0))
        print(f"{name} {what}: {len(np.unique(b[0]))} distinct costs, {distinct} distinct rollouts of {N}")
        assert np.isfinite(b[0]).all() and distinct > N // 2  # (the rows of a wave are different rollouts)
        _same_words(f"{name} {what} costs", a[0], b[0])
        _same_words(f"{name} {what} trace", a[1], b[1])
        assert a[2].tolist() == b[2].tolist(), (name, what, dict(zip(rec.COUNTERS, a[2].tolist())), b[2].tolist())


def test_a_model_set_with_one_hand_geometry_equals_the_single_calls(gpu):
    """Two problems through jh_plan_step_batch_models.  Members that differ in the cube alone keep the tables, and the batch equals jh_plan_step on each member; a member
    with another hand geom size turns the set's tables off, and the batch still equals the single calls (which run each member's own tables)."""
    from judo_amd.device import GpuModel
    from judo_amd.models import load_description, scaled_description
    from tests.test_gpu_model_set import LEAP_A, SetProblems, _settled

    dev = gpu
    desc = load_description("leap_cube")
    x0 = _settled("leap_cube", 60)
    same_hand = [GpuModel(copy.deepcopy(desc), dev), GpuModel(scaled_description(desc, **LEAP_A), dev)]
    p = SetProblems(dev, "leap_cube", same_hand, N=64, K=4, H=8, E=2, seed=5, x0=x0, sigma=NOISE)
    assert p.set.pair_tables()
    p.teeth("mppi")
    p.check("mppi", p.batch_models("mppi"), "one hand geometry")
    other = copy.deepcopy(desc)
    body = {b["name"]: i for i, b in enumerate(other["bodies"])}
    g = next(g for g in other["geoms"] if g["body"] == body["mf_md"] and g["type"] == "box")
    g["size"] = [1.01 * v for v in g["size"]]
    mixed = [same_hand[0], GpuModel(other, dev)]
    p2 = SetProblems(dev, "leap_cube", mixed, N=64, K=4, H=8, E=2, seed=5, x0=x0, sigma=NOISE)
    assert not p2.set.pair_tables()
    p2.check("mppi", p2.batch_models("mppi"), "two hand geometries")
    p2.set.update(1, same_hand[1])  # the odd member replaced: the tables are back
    assert p2.set.pair_tables()
