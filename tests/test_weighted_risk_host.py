"""The plant-weighted risk measure without a device: the numpy restatement (judo_amd.ensemble.aggregate_costs_weighted_host) against an fp64 evaluation of the same
definition and on the properties include/judo_amd.h names, `WorstCase.set_weights` on a stub, `PlantEstimator.apply_risk` on stand-ins, the fleets' refusal of a
weighted member, and every ValueError.

The error bound is the header's: against the fp64 evaluation the restatement stays within 4 (M + 3) 2^-24 of sum(take * |c|) / got -- M products, M - 1 sums, the sums
and differences of the masses and one quotient, each within half an ulp of magnitudes that sum(take * |c|) / got bounds."""

import re
import types

import numpy as np
import pytest

from tests.test_plant_estimator_host import _estimator, _fill

MS = (1, 2, 3, 5, 8, 32)
TAILS = (1.0, 0.5, 0.25, 0.1, 0.03)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _fp64(c, p, tail):
    """The definition in fp64, rollout by rollout: (cost, sum(take * |c|) / got)."""
    c, p, tail = np.asarray(c, np.float64), np.asarray(p, np.float64), float(np.float32(tail))
    cost, mag = np.zeros(c.shape[1]), np.zeros(c.shape[1])
    for r in range(c.shape[1]):
        got = acc = m = 0.0
        for v in sorted(set(c[:, r].tolist()), reverse=True):
            take = min(p[c[:, r] == v].sum(), tail - got)
            if take > 0:
                acc, m, got = acc + take * v, m + take * abs(v), got + take
            if got >= tail:
                break
        cost[r], mag[r] = acc / got, m / got
    return cost, mag


def _inputs(M, N, seed):
    """(M, N) costs of both signs with two-way and three-way ties, and fp32 weights that add up to about 1 with one of them zero (M > 1)."""
    rng = np.random.default_rng(seed)
    c = (rng.standard_normal((M, N)) * 10).astype(np.float32)
    if M >= 2:
        c[1, ::3] = c[0, ::3]
    if M >= 3:
        c[2, ::6] = c[0, ::6]
    p = rng.uniform(0.1, 1.0, M)
    if M > 1:
        p[int(rng.integers(M))] = 0.0
    return c, (p / p.sum()).astype(np.float32)


@pytest.mark.parametrize("M", MS)
def test_restatement_is_within_the_bound_of_an_fp64_evaluation(M):
    from judo_amd.ensemble import aggregate_costs_weighted_host

    for tail in TAILS:
        c, p = _inputs(M, 120, seed=17 * M + int(100 * tail))
        got = aggregate_costs_weighted_host(c, p, tail)
        assert got.dtype == np.float32 and got.shape == (120,)
        want, mag = _fp64(c, p, tail)
        err, bound = np.abs(got.astype(np.float64) - want), 4 * (M + 3) * 2.0**-24 * mag
        assert (err <= bound).all(), (M, tail, float((err / np.maximum(bound, 1e-300)).max()))
    # weights that add up to less than the tail: the divisor is the mass taken, the result the weighted mean of everything
    c, p = _inputs(M, 40, seed=5)
    half = (p * np.float32(0.5)).astype(np.float32)
    want, mag = _fp64(c, half, 1.0)
    mean = (c.astype(np.float64) * half[:, None]).sum(0) / half.astype(np.float64).sum()
    np.testing.assert_allclose(want, mean, rtol=1e-12, atol=1e-12)
    assert (np.abs(aggregate_costs_weighted_host(c, half, 1.0) - want) <= 4 * (M + 3) * 2.0**-24 * mag).all()


@pytest.mark.parametrize("M", MS)
def test_one_hot_weights_return_the_member(M):
    from judo_amd.ensemble import aggregate_costs_weighted_host

    c, _ = _inputs(M, 50, seed=M)
    c[0, 3] = -0.0
    for m in range(M):
        p = np.zeros(M, np.float32)
        p[m] = 1.0
        assert np.array_equal(_bits(aggregate_costs_weighted_host(c, p, 1.0)), _bits(c[m])), m


@pytest.mark.parametrize("M", [1, 2, 4, 8, 32])
def test_uniform_weights_reduce_to_worst_on_distinct_costs(M):
    """M a power of two, weights 1 / M, tail j / M, pairwise distinct costs: bit for bit `aggregate_costs_host(c, worst=j)`."""
    from judo_amd.ensemble import aggregate_costs_host, aggregate_costs_weighted_host

    rng = np.random.default_rng(M)
    c = (rng.standard_normal((M, 200)) * 7).astype(np.float32)
    assert all(len(set(col.tolist())) == M for col in c.T)
    p = np.full(M, 1.0 / M, np.float32)
    for j in range(1, M + 1):
        assert np.array_equal(_bits(aggregate_costs_weighted_host(c, p, j / M)), _bits(aggregate_costs_host(c, j))), j


@pytest.mark.parametrize("M", [2, 3, 5, 8, 32])
def test_permuting_members_with_their_weights_changes_no_bit(M):
    """On pairwise-distinct costs, and where ties have two members (a sum of two weights does not depend on their order)."""
    from judo_amd.ensemble import aggregate_costs_weighted_host

    rng = np.random.default_rng(100 + M)
    c = (rng.standard_normal((M, 90)) * 7).astype(np.float32)
    c[1, ::2] = c[0, ::2]  # two-way ties in every other rollout
    p = rng.uniform(0.0, 1.0, M).astype(np.float32)
    for tail in TAILS:
        want = aggregate_costs_weighted_host(c, p, tail)
        for _ in range(3):
            perm = rng.permutation(M)
            assert np.array_equal(_bits(aggregate_costs_weighted_host(c[perm], p[perm], tail)), _bits(want)), (tail, perm)


def test_inf_and_sentinel_members():
    from judo_amd.ensemble import aggregate_costs_weighted_host

    rng = np.random.default_rng(3)
    c = rng.uniform(0.5, 40.0, (4, 30)).astype(np.float32)
    p = np.array([0.25, 0.0, 0.5, 0.25], np.float32)
    for tail in (1.0, 0.5, 0.1):
        want = aggregate_costs_weighted_host(c, p, tail)
        for big in (np.inf, 3.0e38):
            d = c.copy()
            d[1] = big  # weight zero: changes nothing, and no NaN from 0 * inf
            assert np.array_equal(_bits(aggregate_costs_weighted_host(d, p, tail)), _bits(want)), (tail, big)
    d = c.copy()
    d[2, :10] = np.inf  # positive weight, the largest value: inside every tail
    d[0, 10:20] = 3.0e38
    for tail in (1.0, 0.5, 0.1):
        got = aggregate_costs_weighted_host(d, p, tail)
        assert (got[:10] == np.inf).all() and np.isfinite(got[10:]).all()
        # the sentinel of weight 0.25 is the largest value: take = min(0.25, tail), take * 3.0e38 stays finite, and the tail mean is at least that share of it
        take = np.float32(min(0.25, tail))
        assert (got[10:20] >= np.float32(take * np.float32(3.0e38)) / np.float32(tail)).all()
    # two sentinels in one rollout: the masses taken add up to at most 1, so unlike `worst` = 2 (3.0e38 + 3.0e38 = +inf) the weighted sum stays finite
    e = np.array([[3.0e38], [3.0e38 * 0.99], [1.0]], np.float32)
    got = aggregate_costs_weighted_host(e, np.array([0.6, 0.6, 0.0], np.float32), 1.0)[0]
    assert got == np.float32(np.float32(np.float32(0.6) * e[0, 0]) + np.float32(np.float32(np.float32(1.0) - np.float32(0.6)) * e[1, 0]))
    # a tie of two sentinels is ONE product: (0.5 + 0.5) * 3.0e38 / 1 is the sentinel itself
    e[1] = e[0]
    assert aggregate_costs_weighted_host(e, np.array([0.5, 0.5, 0.0], np.float32), 1.0)[0] == np.float32(3.0e38)


def test_restatement_refusals():
    from judo_amd.ensemble import aggregate_costs_weighted_host as f

    c = np.ones((3, 4), np.float32)
    p = [0.2, 0.3, 0.5]
    assert f(c, p, 1.0).shape == (4,)
    with pytest.raises(ValueError, match=re.escape("member_costs must be (M, N)")):
        f(np.ones(4, np.float32), p, 1.0)
    with pytest.raises(ValueError, match=re.escape("M = 33 outside [1, JH_MAX_ENSEMBLE = 32]")):
        f(np.ones((33, 2), np.float32), [1.0] * 33, 1.0)
    with pytest.raises(ValueError, match="weights is None"):
        f(c, None, 1.0)
    with pytest.raises(ValueError, match="2 weights for M = 3 plants"):
        f(c, [0.5, 0.5], 1.0)
    for bad, idx in (([0.2, -0.1, 0.5], 1), ([np.nan, 0.1, 0.5], 0), ([0.2, 0.1, np.inf], 2)):
        with pytest.raises(ValueError, match=re.escape(f"weights[{idx}] = ") + ".*negative or not finite"):
            f(c, bad, 1.0)
    with pytest.raises(ValueError, match="weights are all zero"):
        f(c, [0.0, 0.0, 0.0], 1.0)
    for tail in (0.0, -0.5, 1.0000001, np.nan, np.inf):
        with pytest.raises(ValueError, match=re.escape("outside (0, 1]")):
            f(c, p, tail)


# ---- WorstCase on a stub ---------------------------------------------------------------------------------------------------------------------------------------
def _stub(M=4, worst=None):
    from judo_amd.plants import PlantSet, WorstCase

    class Stub(WorstCase, PlantSet):
        def __init__(self):
            self._descriptions = [{"i": m} for m in range(M)]
            self.task = types.SimpleNamespace()
            self._init_worst(worst, M)

        def _replace_plant(self, b, description):
            pass

    return Stub()


def test_set_weights_on_a_stub():
    s = _stub(M=4, worst=3)
    assert s.weights is None and s.tail == 0.75  # before any tail was set: worst / M
    s.worst = 1
    assert s.tail == 0.25
    s.set_weights([1, 1, 2, 0])
    assert np.array_equal(s.weights, np.array([0.25, 0.25, 0.5, 0.0], np.float32)) and s.weights.dtype == np.float32 and s.tail == 0.25 and s.worst == 1
    w = np.array([0.3, 0.1, 0.1, 0.2])
    s.set_weights(w, tail=0.1)
    assert np.array_equal(s.weights, (w / w.sum()).astype(np.float32)) and s.tail == float(np.float32(0.1))  # normalised in fp64, then rounded
    got = s.weights
    got[0] = 9.0
    assert s.weights[0] != 9.0  # a copy is handed out
    s.set_weights([1, 0, 0, 0])  # `tail` None keeps the tail
    assert s.tail == float(np.float32(0.1))
    s.set_member(1, {"i": "new"})  # a replaced plant keeps its weight
    assert np.array_equal(s.weights, np.array([1, 0, 0, 0], np.float32)) and s.descriptions[1] == {"i": "new"}
    s.set_weights(None)  # back to the `worst` measure
    assert s.weights is None and s.worst == 1 and s.tail == float(np.float32(0.1))  # (the tail is kept for the next weights)


def test_set_weights_refusals_change_nothing():
    s = _stub(M=3)
    s.set_weights([1, 2, 1], tail=0.5)
    before = s.weights
    for bad in ([1, 1], [1, 1, 1, 1]):
        with pytest.raises(ValueError, match=f"{len(bad)} weights for M = 3 plants"):
            s.set_weights(bad)
    for bad in ([1, -1, 1], [np.nan, 1, 1], [np.inf, 1, 1], [0, 0, 0]):
        with pytest.raises(ValueError, match="non-negative, finite numbers with a positive sum"):
            s.set_weights(bad)
    for tail in (0.0, -1.0, 1.5, np.nan):
        with pytest.raises(ValueError, match=re.escape("outside (0, 1]")):
            s.set_weights([1, 1, 1], tail=tail)
        with pytest.raises(ValueError, match=re.escape("outside (0, 1]")):
            s.set_weights(None, tail=tail)
    assert np.array_equal(s.weights, before) and s.tail == 0.5


def test_every_ensemble_controller_takes_the_weights_from_the_one_place():
    from judo_amd import plants
    from judo_amd.ensemble import EnsembleController
    from judo_amd.fr3_ensemble import FR3EnsembleController
    from judo_amd.fr3_materialized import FR3MaterializedEnsembleController
    from judo_amd.materialized import MaterializedEnsembleController
    from judo_amd.spot_plants import SpotEnsembleController

    for cls in (EnsembleController, FR3EnsembleController, MaterializedEnsembleController, FR3MaterializedEnsembleController, SpotEnsembleController):
        for name in ("set_weights", "weights", "tail", "_aggregate"):
            assert getattr(cls, name) is getattr(plants.WorstCase, name), (cls.__name__, name)
    assert EnsembleController._weighted_entry == "jh_plan_step_ensemble_weighted" and FR3EnsembleController._weighted_entry == "jh_plan_step_ensemble_weighted_phase"


def test_the_entries_are_declared_and_bound():
    import ctypes
    import os

    from judo_amd import _lib
    from tests.conftest import ROOT

    header = open(os.path.join(ROOT, "include", "judo_amd.h")).read()
    L = ctypes.CDLL(_lib.LIB_PATH)
    for name, before in (("jh_ensemble_costs_weighted", "jh_ensemble_costs"), ("jh_plan_step_ensemble_weighted", "jh_plan_step_ensemble"),
                         ("jh_plan_step_ensemble_weighted_phase", "jh_plan_step_ensemble_phase")):
        params = {}
        for n in (name, before):
            m = re.search(rf"\bint\s+{n}\s*\(([^;]*)\)\s*;", header)
            assert m, n
            params[n] = [re.findall(r"[A-Za-z_0-9]+", p)[-1] for p in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",")]
        i = params[before].index("worst")
        assert params[name] == params[before][:i] + ["weights", "tail"] + params[before][i + 1 :]  # `weights`, `tail` where `worst` stands
        res, args = _lib._SIGNATURES[name]
        assert res is ctypes.c_int and len(args) == len(params[name]) and args[i] == ctypes.POINTER(ctypes.c_float) and args[i + 1] is ctypes.c_float
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(L, name)
    assert "aggregate_costs_weighted_host" in header


# ---- apply_risk on stand-ins -----------------------------------------------------------------------------------------------------------------------------------
def test_apply_risk_hands_the_posterior_to_a_worst_case_controller():
    from judo_amd.plants import Assignment

    est = _estimator([[np.inf], [np.inf], [0.0]], horizon=2, windows=4)
    _fill(est, 1)
    ctrl = _stub(M=3, worst=1)
    w = est.apply_risk(ctrl, floor=0.25)
    assert np.array_equal(est.posterior, [0.0, 0.0, 1.0])
    np.testing.assert_allclose(w, [1 / 12, 1 / 12, 10 / 12], rtol=1e-15)
    assert np.array_equal(ctrl.weights, (w / w.sum()).astype(np.float32)) and ctrl.tail == float(np.float32(1) / np.float32(3))
    w = est.apply_risk(ctrl)  # floor 0: the posterior itself
    assert np.array_equal(w, [0.0, 0.0, 1.0]) and np.array_equal(ctrl.weights, np.array([0, 0, 1], np.float32))
    est.apply_risk(ctrl, floor=1.0, tail=0.5)
    assert np.array_equal(ctrl.weights, np.full(3, np.float32(1 / 3))) and ctrl.tail == 0.5
    for floor in (-0.1, 1.1, np.nan):
        with pytest.raises(ValueError, match="floor = "):
            est.apply_risk(ctrl, floor=floor)
    with pytest.raises(ValueError, match="ctrl is a SimpleNamespace, which has no risk measure.*apply_risk needs an EnsembleController"):
        est.apply_risk(types.SimpleNamespace())

    class Randomised(Assignment):
        pass

    with pytest.raises(ValueError, match="ctrl is a Randomised, which has no risk measure.*follows the belief with apply"):
        est.apply_risk(Randomised())
    with pytest.raises(ValueError, match="3 weights for M = 4 plants"):
        est.apply_risk(_stub(M=4))
    with pytest.raises(ValueError, match="plant-weighted risk measure is out of scope"):  # `apply` is what it was
        est.apply(ctrl)


# ---- the fleets --------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fr3", [False, True])
def test_fleets_refuse_a_weighted_member(fr3):
    from judo_amd.ensemble_fleet import EnsembleFleet
    from judo_amd.fr3_ensemble import FR3EnsembleFleet

    cls = FR3EnsembleFleet if fr3 else EnsembleFleet
    assert cls._refuse_weights is EnsembleFleet._refuse_weights
    plain, weighted = _stub(M=3), _stub(M=3)
    weighted.set_weights([1, 2, 3])
    cls._refuse_weights(0, plain)  # a member without weights is taken as before
    with pytest.raises(ValueError, match=r"fleet member 2 has plant weights set \(set_weights\): the fleet launch carries one `worst` per controller"):
        cls._refuse_weights(2, weighted)
    weighted.set_weights(None)
    cls._refuse_weights(2, weighted)
    import inspect

    assert "_refuse_weights(i, c)" in inspect.getsource(EnsembleFleet._check_member)  # (the admission, which ControllerFleet.update_action repeats before every plan step)
