"""The host side of the weighted ensemble fleets, without a device: the numpy restatement of the per-controller risk record against the two restatements it dispatches
to, the packing of the members' records into the fleet's words of their blocks, the admission of weighted members, the makers' refusals, and the three new entries in
the header, the ctypes shim and the built library."""

import copy
import ctypes as C
import os
import re
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _u32(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def _member(M=3, worst=None):
    """A controller's risk measure without a device: `WorstCase` on M descriptions."""
    from judo_amd.plants import PlantSet, WorstCase

    class Stub(WorstCase, PlantSet):
        def __init__(self):
            self._descriptions = [{"i": m} for m in range(M)]
            self.task = types.SimpleNamespace(phase=0)
            self._init_worst(worst, M)

        def _replace_plant(self, b, description):
            pass

    return Stub()


def _descs(task, perturbations):
    from judo_amd.models import scaled_description
    from judo_amd.tasks import get_registered_tasks

    desc = get_registered_tasks()[task][0]().desc
    return [copy.deepcopy(desc)] + [scaled_description(desc, **kw) for kw in perturbations]


# ---- the restatement ---------------------------------------------------------------------------------------------------------------------------------------------
def test_restatement_is_the_two_restatements_controller_by_controller():
    from judo_amd.ensemble import aggregate_costs_host, aggregate_costs_risk_batch_host, aggregate_costs_weighted_host

    rng = np.random.default_rng(5)
    B, M, N = 5, 4, 37
    mc = rng.standard_normal((B, M, N)).astype(np.float32) * 10
    mc[1, 2] = mc[1, 0]  # ties
    mc[3, 1, ::3] = np.inf
    worst = [2, 1, 4, 3, 1]
    risk = np.zeros((B, 1 + M), np.float32)
    risk[0] = [0.0, np.nan, -1.0, np.inf, 7.0]  # a tail word of zero: the weights behind it are not read
    risk[1] = [0.3, 0.1, 0.2, 0.3, 0.4]
    risk[2] = [1.0, 0.0, 0.0, 1.0, 0.0]  # one-hot, tail 1: member 2's row
    risk[3] = [2.0**-20, 0.5, 0.0, 0.25, 0.25]  # (the +inf member has weight zero)
    got = aggregate_costs_risk_batch_host(mc, worst, risk)
    assert got.dtype == np.float32 and got.shape == (B, N)
    for b in range(B):
        want = aggregate_costs_host(mc[b], worst[b]) if risk[b, 0] == 0 else aggregate_costs_weighted_host(mc[b], risk[b, 1:], risk[b, 0])
        assert _u32(got[b]).tobytes() == _u32(want).tobytes(), b
    assert _u32(got[2]).tobytes() == _u32(mc[2, 2]).tobytes()
    assert np.isfinite(got[3]).all()
    # all tail words zero: the counted measure for everybody
    plain = aggregate_costs_risk_batch_host(mc, worst, np.zeros((B, 1 + M), np.float32))
    assert all(_u32(plain[b]).tobytes() == _u32(aggregate_costs_host(mc[b], worst[b])).tobytes() for b in range(B))
    # what it refuses, with the controller named
    with pytest.raises(ValueError, match=re.escape("member_costs must be (B, M, N)")):
        aggregate_costs_risk_batch_host(mc[0], worst, risk)
    with pytest.raises(ValueError, match="4 values of worst for B = 5 controllers"):
        aggregate_costs_risk_batch_host(mc, worst[:4], risk)
    with pytest.raises(ValueError, match=re.escape("risk must be (B, 1 + M) = (5, 5)")):
        aggregate_costs_risk_batch_host(mc, worst, risk[:, :4])
    with pytest.raises(ValueError, match=r"controller 1: worst = 5 outside \[1, M = 4\]"):  # (a weighted controller's `worst` is checked too)
        aggregate_costs_risk_batch_host(mc, [2, 5, 4, 3, 1], risk)
    for word in (-0.5, 1.5, np.nan):
        bad = risk.copy()
        bad[3, 0] = word
        with pytest.raises(ValueError, match=r"controller 3: tail = .* outside \(0, 1\]"):
            aggregate_costs_risk_batch_host(mc, worst, bad)
    bad = risk.copy()
    bad[1, 2] = -0.1
    with pytest.raises(ValueError, match=r"controller 1: weights\[1\] = .*negative or not finite"):
        aggregate_costs_risk_batch_host(mc, worst, bad)
    bad = risk.copy()
    bad[2, 1:] = 0
    with pytest.raises(ValueError, match="controller 2: weights are all zero"):
        aggregate_costs_risk_batch_host(mc, worst, bad)


def test_the_restatement_keeps_the_headers_properties_on_the_gpu_tests_inputs():
    """What tests/test_gpu_ensemble_costs_risk_batch.py feeds the kernel, on the CPU alone: one-hot weights with tail 1 return the member's row exactly, a +inf member of
    weight zero makes no NaN, a three-way tie's group weight is the ascending sum, and uniform weights 1 / M with tail j / M (M a power of two) on pairwise distinct
    costs are bit for bit `worst` = j."""
    from judo_amd.ensemble import aggregate_costs_host, aggregate_costs_weighted_host

    rng = np.random.default_rng(6)
    mc = rng.standard_normal((4, 64)).astype(np.float32)
    for m in range(4):
        hot = np.eye(4, dtype=np.float32)[m]
        assert _u32(aggregate_costs_weighted_host(mc, hot, 1.0)).tobytes() == _u32(mc[m]).tobytes()
    for j in (1, 2, 3, 4):
        assert len({tuple(col) for col in mc.T}) == 64 and all(len(set(col)) == 4 for col in mc.T)
        assert _u32(aggregate_costs_weighted_host(mc, [0.25] * 4, j / 4)).tobytes() == _u32(aggregate_costs_host(mc, j)).tobytes()
    inf = mc.copy()
    inf[1] = np.inf
    assert np.isfinite(aggregate_costs_weighted_host(inf, [0.5, 0.0, 0.25, 0.25], 0.3)).all()
    tie = np.stack([np.full(8, 2.0, np.float32)] * 3 + [np.full(8, 1.0, np.float32)])
    p = np.array([0.1, 0.2, 0.3, 0.4], np.float32)
    ws = np.float32(np.float32(p[0] + p[1]) + p[2])  # the group weight: ascending m
    tail = np.float32(0.9)
    take1 = np.float32(tail - ws)
    want = np.float32(np.float32(np.float32(ws * np.float32(2.0)) + np.float32(take1 * np.float32(1.0))) / np.float32(ws + take1))
    assert (_u32(aggregate_costs_weighted_host(tie, p, tail)) == _u32(want)).all()


# ---- the records in the blocks ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fr3", [False, True])
def test_record_packing(fr3):
    from judo_amd.weighted_fleet import FR3WeightedEnsembleFleet, WeightedEnsembleFleet, risk_record

    cls = FR3WeightedEnsembleFleet if fr3 else WeightedEnsembleFleet
    M, nblk = 3, 11
    cs = [_member(M, worst=2), _member(M, worst=1), _member(M, worst=3)]
    cs[0].set_weights([1, 2, 1], tail=0.5)
    cs[2].set_weights([0, 0, 4])
    cs[2].set_weights(None)  # back to `worst`: the record says so
    fleet = cls.__new__(cls)  # (no device: the class's own pieces on stub members)
    fleet.controllers = cs
    at = 1 if fr3 else 0
    assert fleet._risk_at == at and fleet._block_extra_words == at + 1 + M and fleet._block_extra_at == tuple(range(at + 1))
    stride = nblk + fleet._block_extra_words + 2
    fb = types.SimpleNamespace(host_np=np.full(3 * stride, -9.0, np.float32), blk_stride=stride, nblk=nblk)
    if fr3:
        for i, c in enumerate(cs):
            c.task.phase = i + 1
        fleet._write_phases(fb)
    fleet._write_risk(fb)
    rows = fb.host_np.reshape(3, stride)
    assert (rows[:, :nblk] == -9.0).all() and (rows[:, nblk + at + 1 + M :] == -9.0).all()  # the members' sections and what lies behind the record stay
    if fr3:
        assert rows[:, nblk].tolist() == [1.0, 2.0, 3.0]
    rec = rows[:, nblk + at : nblk + at + 1 + M]
    assert _u32(rec[0]).tobytes() == _u32([0.5, 0.25, 0.5, 0.25]).tobytes()
    assert (rec[1] == 0).all() and (rec[2] == 0).all()
    assert all(_u32(rec[i]).tobytes() == _u32(risk_record(c)).tobytes() for i, c in enumerate(cs))
    cs[1].set_weights([3, 1, 0])  # tail: worst / M = 1 / 3, rounded to fp32
    cs[0].set_weights(None)
    fleet._write_risk(fb)
    assert (rec[0] == 0).all() and _u32(rec[1]).tobytes() == _u32([np.float32(1) / np.float32(3), 0.75, 0.25, 0.0]).tobytes()


def test_launch_step_hands_the_offsets_of_the_fleets_words():
    """`_LaunchStep`'s block run ends in the offsets of the fleet's records: none, the phase word, the risk record, or both."""
    import inspect

    from judo_amd import fleet as F

    src = inspect.getsource(F._LaunchStep.__init__)
    assert "*fb.extra_offsets" in src
    src = inspect.getsource(F._FleetBuffers.__init__)
    assert "self.extra_offsets = tuple(self.nblk + int(at) for at in extra_at) if extra else ()" in src
    assert F.ControllerFleet._block_extra_at == (0,) and F.ControllerFleet._block_extra_words == 0


@pytest.mark.parametrize("fr3", [False, True])
def test_weighted_fleets_accept_what_the_ensemble_fleets_refuse(fr3):
    from judo_amd.ensemble_fleet import EnsembleFleet
    from judo_amd.fr3_ensemble import FR3EnsembleFleet
    from judo_amd.weighted_fleet import FR3WeightedEnsembleFleet, WeightedEnsembleFleet

    old, new = (FR3EnsembleFleet, FR3WeightedEnsembleFleet) if fr3 else (EnsembleFleet, WeightedEnsembleFleet)
    assert issubclass(new, old) and new._check_member is old._check_member  # every other admission rule is inherited
    c = _member(3)
    c.set_weights([1, 2, 3])
    with pytest.raises(ValueError, match=r"fleet member 1 has plant weights set \(set_weights\): the fleet launch carries one `worst` per controller.*WeightedEnsembleFleet"):
        old._refuse_weights(1, c)
    assert new._refuse_weights(1, c) is None
    assert new._refuse_weights(1, _member(3)) is None


# ---- the makers -----------------------------------------------------------------------------------------------------------------------------------------------------
def test_makers_raise_before_any_device_use():
    from judo_amd.weighted_fleet import fleet_tails, make_fr3_weighted_ensemble_fleet, make_weighted_ensemble_fleet

    cart = _descs("cartpole", [dict(body_mass={"pole": 1.5}), dict(body_mass={"pole": 0.7})])
    with pytest.raises(ValueError, match="Task nope not found"):
        make_weighted_ensemble_fleet("nope", "mppi", 2, cart)
    with pytest.raises(ValueError, match="at least one controller"):
        make_weighted_ensemble_fleet("cartpole", "mppi", 0, cart)
    with pytest.raises(ValueError, match="3 lists of descriptions for a fleet of 2"):
        make_weighted_ensemble_fleet("cartpole", "mppi", 2, [cart, cart, cart])
    with pytest.raises(ValueError, match=r"fleet member 1: worst = 4 outside \[1, M = 3\]"):
        make_weighted_ensemble_fleet("cartpole", "mppi", 2, cart, worst=[1, 4])
    with pytest.raises(ValueError, match="2 weights for M = 3 plants"):
        make_weighted_ensemble_fleet("cartpole", "mppi", 2, cart, weights=[1, 2])
    with pytest.raises(ValueError, match="3 lists of weights for a fleet of 2"):
        make_weighted_ensemble_fleet("cartpole", "mppi", 2, cart, weights=[[1, 2, 3]] * 3)
    with pytest.raises(ValueError, match="fleet member 1: 2 weights for M = 3 plants"):
        make_weighted_ensemble_fleet("cartpole", "mppi", 2, cart, weights=[[1, 2, 3], [1, 2]])
    with pytest.raises(ValueError, match="fleet member 1: weights must be non-negative, finite numbers with a positive sum"):
        make_weighted_ensemble_fleet("cartpole", "mppi", 2, cart, weights=[[1, 2, 3], [1, -2, 3]])
    with pytest.raises(ValueError, match="fleet member 0: weights must be non-negative"):
        make_weighted_ensemble_fleet("cartpole", "mppi", 2, cart, weights=[0, 0, 0])
    with pytest.raises(ValueError, match="3 values of tail for a fleet of 2"):
        make_weighted_ensemble_fleet("cartpole", "mppi", 2, cart, tail=[0.5, 0.5, 0.5])
    for bad in (0.0, 1.5, float("nan")):
        with pytest.raises(ValueError, match=r"fleet member 1: tail = .* outside \(0, 1\]"):
            make_weighted_ensemble_fleet("cartpole", "mppi", 2, cart, tail=[0.5, bad])
    assert fleet_tails(3, None) == [None] * 3 and fleet_tails(2, 0.25) == [0.25, 0.25] and fleet_tails(2, (1.0, 0.5)) == [1.0, 0.5]
    with pytest.raises(ValueError, match="Optimizer nope not found"):
        make_fr3_weighted_ensemble_fleet("nope", 2, cart)
    from judo_amd.tasks import FR3Pick

    arm = FR3Pick().desc
    with pytest.raises(ValueError, match="fleet member 0: description 0 differs from the task in self_collision"):
        make_fr3_weighted_ensemble_fleet("mppi", 2, [arm, arm], self_collision=True)
    with pytest.raises(ValueError, match="1 weights for M = 2 plants"):
        make_fr3_weighted_ensemble_fleet("mppi", 2, [arm, arm], weights=[1.0])
    with pytest.raises(ValueError, match=r"fleet member 0: tail = .* outside \(0, 1\]"):
        make_fr3_weighted_ensemble_fleet("mppi", 2, [arm, arm], tail=2.0)


# ---- the entries -----------------------------------------------------------------------------------------------------------------------------------------------------
_CTYPES = {"int": C.c_int, "float": C.c_float, "size_t": C.c_size_t, "constint*": C.POINTER(C.c_int)}


def _declared(header, name):
    m = re.search(rf"\bint\s+{name}\s*\(([^;]*)\);", header)
    assert m, f"include/judo_amd.h does not declare {name}"
    return [p.strip() for p in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",")]


def test_the_three_entries_are_declared_bound_and_built():
    """Fails without the feature: the header, the shim and the built library all lack the symbols."""
    from judo_amd import _lib

    header = open(os.path.join(ROOT, "include", "judo_amd.h")).read()
    assert "The batched entries have no weighted form" not in header
    L = _lib.lib()
    for name, n in (("jh_ensemble_costs_risk_batch", 11), ("jh_plan_step_ensemble_batch_risk", 32), ("jh_plan_step_ensemble_batch_phases_risk", 33)):
        params = _declared(header, name)
        restype, argtypes = _lib._SIGNATURES[name]
        assert restype is C.c_int and len(params) == len(argtypes) == n and name in _lib.EXPORTED_SYMBOLS, name
        for p, t in zip(params, argtypes):  # scalars and the host array by type; every pointer to device or handle memory travels as an address
            kind = re.sub(r"\s*\w+$", "", p).replace(" ", "")
            assert t is _CTYPES.get(kind, C.c_void_p), (name, p, t)
        fn = getattr(L, name)  # the built library exports it
        assert fn.restype is C.c_int and list(fn.argtypes) == list(argtypes)
    base = _declared(header, "jh_plan_step_ensemble_batch")
    risk = _declared(header, "jh_plan_step_ensemble_batch_risk")
    assert risk[:11] == base[:11] and risk[11] == "int o_risk" and risk[12:] == base[11:]  # `o_risk` behind o_lohi, nothing else
    base = _declared(header, "jh_plan_step_ensemble_batch_phases")
    risk = _declared(header, "jh_plan_step_ensemble_batch_phases_risk")
    assert risk[:12] == base[:12] and base[11] == "int o_phase" and risk[12] == "int o_risk" and risk[13:] == base[12:]  # ... behind o_phase
    # a null pointer is refused by name without a device
    assert L.jh_ensemble_costs_risk_batch(None, 1, 1, 1, 1, None, 2, None, None, 1, None) == -1
    assert "ensemble_costs_risk_batch: member_costs is a null pointer" in L.jh_last_error().decode()
