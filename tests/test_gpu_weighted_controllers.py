"""The plant-weighted risk measure through the five ensemble controller classes (`plants.WorstCase.set_weights`): EnsembleController and FR3EnsembleController pick the
weighted plan step, MaterializedEnsembleController, FR3MaterializedEnsembleController and SpotEnsembleController the weighted aggregation of their materialise path.
Each class runs at the shape of its own test file.  Everything compared is compared bit for bit."""

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

KINDS = ["fused", "fr3", "materialized", "fr3_materialized", "spot"]
ENTRY = {"fused": ("jh_plan_step_ensemble_weighted", "jh_plan_step_ensemble"), "fr3": ("jh_plan_step_ensemble_weighted_phase", "jh_plan_step_ensemble_phase"),
         "materialized": ("jh_ensemble_costs_weighted", "jh_ensemble_costs"), "fr3_materialized": ("jh_ensemble_costs_weighted", "jh_ensemble_costs"),
         "spot": ("jh_ensemble_costs_weighted", "jh_ensemble_costs")}


class Kit:
    """One controller class at its smallest existing test shape: `descs(M)` distinct plants, `ensemble(descs, worst)` and `plain(desc)` configured controllers from
    one seed and state (the plain one is the controller the class's own tests compare a member with), `set_state(c, step)`."""

    def __init__(self, kind):
        self.kind = kind
        getattr(self, "_" + kind)()

    def _cartpole_descs(self, M):
        from judo_amd.models import scaled_description
        from tests.test_gpu_ensemble_controller import _descriptions
        from tests.test_gpu_model_set import CARTPOLE

        d = _descriptions("cartpole", CARTPOLE)
        return (d + [scaled_description(d[0], body_mass={"pole": 2.0, "cart": 0.8})])[:M]

    def _fused(self):
        from judo_amd.ensemble import make_ensemble_controller
        from tests import test_gpu_ensemble_controller as T

        def ready(c):
            T._configure(c, "mppi")
            return c

        self.descs = self._cartpole_descs
        self.ensemble = lambda descs, worst=None: ready(make_ensemble_controller("cartpole", "mppi", descs, worst=worst))
        self.plain = lambda desc: ready(T._plain_on("cartpole", "mppi", desc))
        self.set_state = T._set_state

    def _fr3(self):
        from judo_amd.fr3_ensemble import make_fr3_ensemble_controller
        from tests.test_fr3_plants_host import plants
        from tests.test_gpu_fr3_fleet import _configure, _set_state
        from tests.test_gpu_fr3_plants import _lone_on

        def ready(c):
            _configure(c, 5, n=16)
            _set_state(c, 0, 0)
            return c

        self.descs = lambda M: list(plants()[:M])
        self.ensemble = lambda descs, worst=None: ready(make_fr3_ensemble_controller("mppi", descs, worst=worst))
        self.plain = lambda desc: ready(_lone_on(desc, "mppi"))
        self.set_state = lambda c, step: _set_state(c, 0, step)

    def _materialized(self):
        from tests import test_gpu_materialized_controllers as T

        self.descs = self._cartpole_descs
        self.ensemble = lambda descs, worst=None: T._ensemble("cartpole", "mppi", descs, worst=worst)
        self.plain = lambda desc: T._plain("cartpole", "mppi", desc)
        self.set_state = T._set_state

    def _fr3_materialized(self):
        from tests import test_gpu_fr3_materialized_controllers as T
        from tests.test_fr3_plants_host import plants
        from tests.test_gpu_fr3_fleet import _set_state

        def ready(c):
            _set_state(c, 0, 0)
            return c

        self.descs = lambda M: list(plants()[:M])
        self.ensemble = lambda descs, worst=None: ready(T._ensemble("mppi", descs, worst=worst))
        self.plain = lambda desc: ready(T._plain("mppi", desc))
        self.set_state = lambda c, step: _set_state(c, 0, step)

    def _spot(self):
        from tests import test_gpu_spot_plant_controllers as T

        self.descs = lambda M: T._descs("spot_box_push", M)
        self.ensemble = lambda descs, worst=None: T._ensemble("spot_box_push", "mppi", descs, worst=worst)
        self.plain = lambda desc: T._configure(T._plain("spot_box_push", "mppi", desc), "mppi")
        self.set_state = T._set_state


def _same(x, y, what):
    x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
    assert x.shape == y.shape and x.dtype == y.dtype, what
    assert x.tobytes() == y.tobytes(), f"{what} differs (max |d| = {np.abs(x - y).max():.3e})"


def _one_hot(M, m):
    return [1.0 if i == m else 0.0 for i in range(M)]


@pytest.mark.parametrize("kind", KINDS)
def test_one_hot_weights_plan_on_that_plant(gpu, kind):
    """M = 3 distinct plants, `set_weights(one_hot(m), tail=1.0)`: the rewards are member m's and the nominal is that of a plain controller on plant m."""
    kit = Kit(kind)
    descs = kit.descs(3)
    for m in (2, 0) if kind != "spot" else (2,):
        ens, plain = kit.ensemble(descs), kit.plain(descs[m])
        ens.set_weights(_one_hot(3, m), tail=1.0)
        assert ens.weights.tolist() == _one_hot(3, m) and ens.tail == 1.0 and ens.worst == 3
        ens.update_action()
        plain.update_action()
        mr = ens.member_rewards
        assert len({mr[i].tobytes() for i in range(3)}) == 3  # the plants matter
        _same(np.asarray(ens.rewards, np.float64), mr[m], f"{kind}: rewards against member_rewards[{m}]")
        _same(np.asarray(ens.rewards, np.float64), np.asarray(plain.rewards, np.float64), f"{kind}: rewards against the plain controller on plant {m}")
        _same(ens.nominal_knots, plain.nominal_knots, f"{kind}: nominal against the plain controller on plant {m}")


@pytest.mark.parametrize("kind", ["fused", "materialized"])
def test_uniform_weights_are_the_worst_measure(gpu, kind):
    """M = 4 cartpole plants whose member costs are pairwise distinct in every rollout: uniform weights with tail = j / 4 give the costs and the nominal of `worst` = j.
    Two controllers in lockstep from one seed, j = 1, 2, 3, 4 over four plan steps."""
    kit = Kit(kind)
    descs = kit.descs(4)
    a, b = kit.ensemble(descs), kit.ensemble(descs)
    for step, j in enumerate((1, 2, 3, 4)):
        a.worst = j
        b.set_weights([1, 1, 1, 1], tail=j / 4)
        assert b.weights.tolist() == [0.25] * 4 and b.tail == j / 4
        for c in (a, b):
            kit.set_state(c, step)
            c.update_action()
        mc = a.member_costs
        assert all(len(set(col.tolist())) == 4 for col in mc.T), "a rollout with equal member costs: choose other plants"
        _same(b.member_costs, mc, f"{kind} j={j}: member costs")
        _same(np.asarray(b.rewards), np.asarray(a.rewards), f"{kind} j={j}: rewards")
        _same(b.nominal_knots, a.nominal_knots, f"{kind} j={j}: nominal")


@pytest.mark.parametrize("kind", KINDS)
def test_weights_and_tail_take_effect_at_the_next_plan_step(gpu, kind, monkeypatch):
    """One controller over three plants: weights and tail changed between plan steps are the measure of the next one (the rewards are the negated restatement on that
    step's member costs, through the weighted entry, one call per iteration), and `set_weights(None)` returns to the `worst` measure and the unweighted entry."""
    from judo_amd import _lib
    from judo_amd.ensemble import aggregate_costs_host, aggregate_costs_weighted_host

    L = _lib.lib()
    calls = {name: 0 for name in ENTRY[kind]}

    def counted(name):
        fn = getattr(L, name)

        def wrapper(*a):
            calls[name] += 1
            return fn(*a)

        return wrapper

    for name in calls:
        monkeypatch.setattr(L, name, counted(name))
    weighted, unweighted = ENTRY[kind]
    kit = Kit(kind)
    ens = kit.ensemble(kit.descs(3), worst=2)
    ens.controller_cfg.max_opt_iters = 1
    seen = []
    for step, (w, tail) in enumerate((([0.2, 0.5, 0.3], 0.5), ([3.0, 1.0, 0.0], 0.25), ([1.0, 1.0, 2.0], None), (None, None))):
        ens.set_weights(w, tail) if tail is not None else ens.set_weights(w)
        before = dict(calls)
        kit.set_state(ens, step)
        ens.update_action()
        mc = ens.member_costs
        if w is None:
            assert ens.weights is None and ens.worst == 2
            want = aggregate_costs_host(mc, 2)
            assert calls[unweighted] == before[unweighted] + 1 and calls[weighted] == before[weighted]
        else:
            p = (np.asarray(w, np.float64) / np.sum(w)).astype(np.float32)
            assert np.array_equal(ens.weights, p) and ens.tail == (0.5 if step == 0 else 0.25)
            want = aggregate_costs_weighted_host(mc, p, ens.tail)
            assert calls[weighted] == before[weighted] + 1 and calls[unweighted] == before[unweighted]
            assert (want != aggregate_costs_host(mc, 2)).any()
        _same(np.asarray(ens.rewards, np.float64), -want.astype(np.float64), f"{kind} step {step}: rewards")
        _same(ens.costs_device.cpu().numpy(), want, f"{kind} step {step}: costs")
        seen.append(want.tobytes())
    assert len(set(seen)) == 4


def test_set_weights_none_restores_the_old_bits(gpu):
    """Two fused controllers in lockstep: one goes through `set_weights(...)` and back to None between two plan steps without planning; both plan the same bits."""
    kit = Kit("fused")
    descs = kit.descs(3)
    a, b = kit.ensemble(descs, worst=2), kit.ensemble(descs, worst=2)
    for step in range(2):
        b.set_weights([0.1, 0.2, 0.7], tail=0.3)
        b.set_weights(None)
        for c in (a, b):
            kit.set_state(c, step)
            c.update_action()
        _same(b.member_costs, a.member_costs, f"step {step}: member costs")
        _same(np.asarray(b.rewards), np.asarray(a.rewards), f"step {step}: rewards")
        _same(b.nominal_knots, a.nominal_knots, f"step {step}: nominal")


def test_fleet_refuses_a_weighted_member(gpu):
    from judo_amd.ensemble_fleet import EnsembleFleet

    kit = Kit("fused")
    descs = kit.descs(3)
    a, b = kit.ensemble(descs), kit.ensemble(descs)
    b.set_weights([1, 2, 3])
    with pytest.raises(ValueError, match=r"fleet member 1 has plant weights set.*one `worst` per controller"):
        EnsembleFleet([a, b])
    b.set_weights(None)
    fleet = EnsembleFleet([a, b])  # members without weights are taken as before
    fleet.update_action()
    a.set_weights([1, 2, 3])  # ... and weights set on a member of a fleet stop the fleet's next plan step
    with pytest.raises(ValueError, match=r"fleet member 0 has plant weights set"):
        fleet.update_action()


def test_closed_loop_on_cartpole(gpu):
    """The truth is plant 2: the estimator on an EnsembleController's three plants finds it from 2 * horizon observed steps, `apply_risk(ctrl, floor=0.1)` sets the
    weights of the formula, and the next plan step's costs are the restatement with those weights."""
    import torch

    from judo_amd.ensemble import aggregate_costs_weighted_host, make_ensemble_controller
    from judo_amd.identify import PlantEstimator
    from tests import test_gpu_materialize_plants as closed
    from tests.test_gpu_plant_estimator import W, _cartpole_descriptions, _configure, _reference

    ref = _reference("cartpole")
    H = ref["H"]
    ctrl = make_ensemble_controller("cartpole", "mppi", _cartpole_descriptions(), worst=1)
    _configure(ctrl)
    ctrl.update_action()
    est = PlantEstimator.for_controller(ctrl, horizon=H, windows=W, state_sigma=1e-4)
    truth = ref["models"][2]
    x = torch.from_numpy(closed._x0("cartpole", 1, 9)[0]).to(gpu)
    us = torch.from_numpy(closed._controls("cartpole", 1, 2 * H, 10)).to(gpu)
    for t in range(2 * H):
        u = us[:, t : t + 1].contiguous()
        x_next = closed._single(truth, x, 0, u, want_sensors=False)[0][0, 0].clone()
        est.observe_step(x, u[0, 0], x_next)
        x = x_next
    assert len(est) == 2 and est.pending_steps == 0
    w = est.apply_risk(ctrl, floor=0.1)
    assert est.map == 2 and est.posterior[2] > 0.99, (est.posterior, est.errors)
    formula = 0.9 * est.posterior + 0.1 / 3
    assert np.array_equal(w, formula) and np.array_equal(ctrl.weights, (formula / formula.sum()).astype(np.float32))
    assert ctrl.tail == float(np.float32(1) / np.float32(3)) and ctrl.worst == 1  # (`tail` None: worst / M)
    ctrl.update_action()
    torch.cuda.synchronize()
    mc = ctrl.member_costs
    want = aggregate_costs_weighted_host(mc, ctrl.weights, ctrl.tail)
    _same(ctrl.costs_device.cpu().numpy(), want, "costs after apply_risk")
    _same(np.asarray(ctrl.rewards, np.float64), -want.astype(np.float64), "rewards after apply_risk")
    assert (want != mc.max(axis=0)).any() and np.isfinite(ctrl.nominal_knots).all()  # no longer the worst case over all three plants
    with pytest.raises(ValueError, match="plant-weighted risk measure is out of scope"):  # `apply` refuses an ensemble controller as before
        est.apply(ctrl)
