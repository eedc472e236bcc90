"""judo_amd.simulation without a device: the numpy restatements of jh_plant_controls and jh_plant_reports, the splines of a segment, and `GpuSimulation`, `PlantFleet`
and `ClosedLoop` on stand-ins -- hook order, pause, `steps_per_plan`, the `plan_delay` split, every ValueError, the Spot refusal by name.

The stand-ins live on the CPU device, as in tests/test_plant_reports_host.py: everything up to the library call is host work."""

import ctypes
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

KINDS = ["zero", "linear", "cubic"]


# ---- the C boundary ------------------------------------------------------------------------------------------------------------------------------------------------
def test_header_table_and_library_agree_on_the_entries():
    from judo_amd import _lib
    from tests.conftest import ROOT

    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "judo_amd.h")).read(), flags=re.S)
    want = {
        "jh_plant_controls": ["W", "knots", "knot_stride", "ctrl_lo_hi", "B", "S", "K", "nu", "step0", "ld_steps", "controls", "stream"],
        "jh_plant_reports": ["states", "sensors", "B", "S", "nx", "ns", "count", "every", "noise", "sigma", "column_mask", "reports", "noise_sens", "sigma_sens",
                             "column_mask_sens", "reports_sens", "x", "stream"],
        "jh_plants_advance": ["set", "truth", "B", "x", "W", "knots", "knot_stride", "K", "ctrl_lo_hi", "step0", "S", "controls", "states", "sensors", "count", "every", "noise",
                              "sigma", "column_mask", "reports", "noise_sens", "sigma_sens", "column_mask_sens", "reports_sens", "stream"],
    }
    built = ctypes.CDLL(_lib.LIB_PATH)
    for name, params in want.items():
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", header)
        assert m, f"{name} is not declared"
        assert [re.findall(r"[A-Za-z_0-9]+", p)[-1] for p in m.group(1).split(",")] == params
        res, args = _lib._SIGNATURES[name]
        assert res is ctypes.c_int and len(args) == len(params) and name in _lib.EXPORTED_SYMBOLS and hasattr(built, name), name
        assert args[params.index("knot_stride")] is ctypes.c_size_t if "knot_stride" in params else True
        assert args[params.index("count")] == ctypes.POINTER(ctypes.c_int) if "count" in params else True
    from __graft_entry__ import HIP_SOURCES

    assert "jh_plants.hip" in HIP_SOURCES


# ---- plant_controls_host -------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [4, 7])
@pytest.mark.parametrize("kind", KINDS)
def test_controls_restatement_against_the_spline_in_fp64(kind, K):
    """Per entry |fp32 - fp64| <= (K + 1) * 2**-24 * sum_k |W_k| |knot_k|: the knots are fp32 numbers in both evaluations, so the fp32 one rounds each weight (1), each
    product (1) and K - 1 sums -- K + 1 roundings of at most 2**-24 relative each on a quantity bounded by the sum of the terms' magnitudes.  Queries in front of, on
    and behind the knot span, B = 3 plants with knot grids shifted against one another."""
    from judo_amd.simulation import plant_controls_host
    from judo_amd.spline import evaluate, spline_weights

    rng = np.random.default_rng(K)
    B, nu = 3, 5
    grids = [0.13 * b + np.linspace(0.0, 0.6, K) for b in range(B)]
    q = np.concatenate([[-0.2, -1e-9], grids[0][[0, 1, K - 1]], [0.05, 0.31, 0.599], grids[1][[1, 2]], [0.95, 3.0]])
    knots = rng.standard_normal((B, K, nu)).astype(np.float32)
    W64 = np.stack([spline_weights(kind, grids[b], q) for b in range(B)])
    got = plant_controls_host(W64.astype(np.float32), knots)
    assert got.dtype == np.float32 and got.shape == (B, len(q), nu)
    for b in range(B):
        ref = evaluate(kind, grids[b], knots[b].astype(np.float64), q)
        bound = (K + 1) * 2.0**-24 * np.einsum("sk,ku->su", np.abs(W64[b]), np.abs(knots[b].astype(np.float64)))
        err = np.abs(got[b].astype(np.float64) - ref)
        assert (err <= bound).all(), (kind, K, b, float((err - bound).max()))
        if kind != "cubic":  # in front of and behind the span the first and the last knot are held, exactly
            assert np.array_equal(got[b][q < grids[b][0]], np.broadcast_to(knots[b, 0], (int((q < grids[b][0]).sum()), nu)))
            assert np.array_equal(got[b][q > grids[b][-1]], np.broadcast_to(knots[b, -1], (int((q > grids[b][-1]).sum()), nu)))


def test_controls_restatement_order_clip_and_refusals():
    from judo_amd.simulation import plant_controls_host

    # the order of the sum: (a * 1 + b * 1) + c * 1 with a + b exact and c lost, against any other order
    W = np.ones((1, 1, 3), dtype=np.float32)
    knots = np.array([[[2.0**24], [-(2.0**24)], [1.0]]], dtype=np.float32)
    assert plant_controls_host(W, knots)[0, 0, 0] == 1.0
    assert plant_controls_host(W, knots[:, [0, 2, 1]])[0, 0, 0] == 0.0  # (2^24 + 1 rounds to 2^24)
    # no fused multiply-add: 3 * (1/3 rounded) - 1 is exactly 0 when the product is rounded first
    third = np.float32(1.0) / np.float32(3.0)
    assert plant_controls_host(np.array([[[3.0, 1.0]]], np.float32), np.array([[[third], [-1.0]]], np.float32))[0, 0, 0] == np.float32(np.float32(3.0) * third) - np.float32(1.0)
    # the clip, on the bits: -0.0 lies below +0.0, a NaN passes through
    u = plant_controls_host(np.ones((1, 4, 1), np.float32), np.array([[[-3.0, -0.0, 0.5, np.nan]]], np.float32).reshape(1, 1, 4), [0.0, 0.0, 0.0, 0.0, 1.0, 1.0, 0.25, 1.0])
    assert u.shape == (1, 4, 4) and u[0, 0].view(np.uint32).tolist() == [0, 0, np.float32(0.25).view(np.uint32), 0x7FC00000]
    # 2-D forms, and the refusals
    assert plant_controls_host(np.ones((2, 3)), np.ones((3, 2))).shape == (1, 2, 2)
    for bad in (dict(W=np.ones((1, 2, 3)), knots=np.ones((1, 4, 2))), dict(W=np.ones((2, 2, 3)), knots=np.ones((1, 3, 2))), dict(W=np.ones((1, 2, 64)), knots=np.ones((1, 64, 9))),
                dict(W=np.ones((1, 2, 3)), knots=np.ones((1, 3, 2)), ctrl_lo_hi=[0.0, 1.0, 2.0])):
        with pytest.raises(ValueError):
            plant_controls_host(**bad)


# ---- plant_reports_host --------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("every", [1, 2, 3])
def test_the_report_stride_carries_across_segments(every):
    """S = 5, two segments: over both, exactly the steps whose running number -- 1 for the first step the plant ever took -- divides by `every` are reported."""
    from judo_amd.simulation import plant_reports_host, reported_steps

    rng = np.random.default_rng(every)
    B, S, nx = 2, 5, 4
    count = np.array([0, 3])  # plant 1 has taken three steps before
    got = []
    for seg in range(2):
        states = rng.standard_normal((B, S, nx)).astype(np.float32)
        rep, carry = plant_reports_host(states, count, every=every)
        assert rep.dtype == np.float32 and np.array_equal(carry, states[:, -1])
        want_steps = np.array([[(count[b] + s + 1) % every == 0 for s in range(S)] for b in range(B)])
        assert np.array_equal(reported_steps(count, S, every), want_steps)
        assert np.array_equal(np.isnan(rep), np.broadcast_to(~want_steps[:, :, None], rep.shape))  # NaN exactly where nothing is reported
        assert np.array_equal(rep[want_steps], states[want_steps])  # ... and the state, bit for bit, elsewhere
        got.append(want_steps)
        count = count + S
    for b, before in enumerate((0, 3)):
        numbers = before + 1 + np.flatnonzero(np.concatenate([g[b] for g in got]))
        assert numbers.tolist() == [n for n in range(before + 1, before + 2 * S + 1) if n % every == 0]


def test_reports_mask_noise_and_carry():
    from judo_amd.simulation import plant_reports_host

    rng = np.random.default_rng(0)
    B, S, nx, nq = 3, 5, 6, 4
    states = rng.standard_normal((B, S, nx)).astype(np.float32)
    noise = rng.standard_normal((B, S, nx)).astype(np.float32)
    sigma = rng.uniform(0.01, 0.1, nx).astype(np.float32)
    cols = np.arange(nx) < nq
    rep, carry = plant_reports_host(states, [1, 0, 4], every=2, columns=cols, sigma=sigma, noise=noise)
    steps = np.array([[(c + s + 1) % 2 == 0 for s in range(S)] for c in (1, 0, 4)])
    shown = steps[:, :, None] & cols[None, None, :]
    assert np.array_equal(np.isnan(rep), ~shown)
    want = states + (sigma * noise).astype(np.float32)  # the product rounded, then the sum rounded
    assert np.array_equal(rep[shown].view(np.uint32), want[shown].view(np.uint32)) and (rep[shown] != states[shown]).any()
    assert np.array_equal(carry.view(np.uint32), states[:, -1].view(np.uint32))  # the exact state, never the noisy one
    full, _ = plant_reports_host(states, [0, 0, 0])
    assert np.array_equal(full.view(np.uint32), states.view(np.uint32))  # everything reported, no noise: the states bit for bit
    zero, _ = plant_reports_host(states, [0, 0, 0], sigma=np.zeros(nx), noise=noise)
    assert np.array_equal(zero, states)
    for bad in (dict(count=[0, 0]), dict(count=[0, 0, 0], every=0), dict(count=[0, -1, 0]), dict(count=[0, 0, 0], columns=[True] * 5),
                dict(count=[0, 0, 0], sigma=np.ones(5), noise=noise), dict(count=[0, 0, 0], sigma=np.ones(nx), noise=noise[:, :4])):
        with pytest.raises(ValueError):
            plant_reports_host(states, **bad)
    with pytest.raises(ValueError):
        plant_reports_host(states[0], [0])


# ---- the splines of a segment --------------------------------------------------------------------------------------------------------------------------------------
def _spline(kind, t0, K, nu, seed):
    from judo_amd.structs import SplineData

    return SplineData(t0 + np.linspace(0.0, 0.4, K), np.random.default_rng(seed).standard_normal((K, nu)), kind)


def test_the_plan_delay_split():
    """With plan_delay = L the first L steps of a segment follow the old splines and the rest the new ones, each plant at its own clock."""
    from judo_amd.simulation import plant_controls_host, segment_rows
    from judo_amd.spline import evaluate

    dt, S, L, times = 0.02, 5, 2, np.array([0.1, 0.3, 0.14])
    new = [_spline("cubic", t, 4, 2, 10 + b) for b, t in enumerate(times)]
    old = [_spline("linear", t - 0.1, 6, 2, 20 + b) for b, t in enumerate(times)]  # (another kind, another K: the old range is a launch of its own)
    o, n = segment_rows(new, old, times, dt, S, L)
    assert o[0].shape == (3, L, 6) and o[1].shape == (3, 6, 2) and n[0].shape == (3, S - L, 4) and n[1].shape == (3, 4, 2) and all(a.dtype == np.float32 for a in o + n)
    u = np.concatenate([plant_controls_host(*o), plant_controls_host(*n)], axis=1)
    for b, t in enumerate(times):
        q = t + dt * np.arange(S)
        want = np.concatenate([evaluate("linear", old[b].t, old[b].x, q[:L]), evaluate("cubic", new[b].t, new[b].x, q[L:])])
        np.testing.assert_allclose(u[b], want, rtol=0, atol=2e-6)
    none, whole = segment_rows(new, None, times, dt, S, 0)
    assert none is None and whole[0].shape == (3, S, 4)
    ctrl = SimpleNamespace(spline_data=new[0])  # a controller stands for its spline; a fleet for its controllers'
    assert np.array_equal(segment_rows(SimpleNamespace(controllers=[ctrl]), None, times[:1], dt, S, 0)[1][0], whole[0][:1])
    for bad, msg in ((dict(steps=0), "steps = 0"), (dict(plan_delay=5), "plan_delay = 5"), (dict(plan_delay=-1), "plan_delay = -1"), (dict(plan_delay=2, old_splines=None), "needs old_splines"),
                     (dict(splines=new[:2]), "2 splines for B = 3"), (dict(splines=new[:2] + [_spline("zero", 0.0, 5, 2, 0)]), "one shape"),
                     (dict(splines=[_spline("zero", 0.0, 40, 16, 0)] * 3), "JH_MAX_KNOT_DIM"), (dict(splines=[1, 2, 3]), "SplineData")):
        kw = dict(splines=new, old_splines=old, times=times, dt=dt, steps=S, plan_delay=0)
        kw.update(bad)
        with pytest.raises(ValueError, match=msg):
            segment_rows(**kw)


# ---- PlantFleet on a stand-in set ----------------------------------------------------------------------------------------------------------------------------------
def _cpu_set(M=3, nq=2, nv=2, nu=1, ns=3):
    import torch

    return SimpleNamespace(models=[SimpleNamespace(nq=nq, nv=nv, nx=nq + nv, nu=nu, ns=ns, dt=0.01, device=torch.device("cpu")) for _ in range(M)], handle=None)


def test_plant_fleet_checks_without_a_device():
    from judo_amd.simulation import PlantFleet

    mset = _cpu_set()
    f = PlantFleet(mset, [2, 0, 2], np.arange(4.0), time=1.0)
    assert len(f) == 3 and f.truth == [2, 0, 2] and f.x_host().shape == (3, 4) and np.array_equal(f.x_host()[1], np.arange(4.0)) and f.time.tolist() == [1.0, 1.0, 1.0]
    f.set_state(np.ones((3, 4)), time=0.5)
    assert f.x_host().sum() == 12 and f.time.tolist() == [0.5] * 3 and f.steps_taken.tolist() == [0, 0, 0]
    for truth, x0, kw, msg in (([0, 3], np.zeros(4), {}, r"plant_of_block\[1\] = 3"), ([], np.zeros(4), {}, "0 blocks"), ([0, 1], np.zeros((3, 4)), {}, "x0 must be"),
                               ([0], np.full(4, np.nan), {}, "x0 must be"), ([0], np.zeros(4), dict(ctrl_lo_hi=[0.0]), "ctrl_lo_hi")):
        with pytest.raises(ValueError, match=msg):
            PlantFleet(mset, truth, x0, **kw)
    with pytest.raises(ValueError, match="GpuModelSet"):
        PlantFleet(object(), [0], np.zeros(4))
    f.reports(every=2, columns=range(2), state_sigma=0.1, sensor_sigma=[0.1, 0.2, 0.0], seed=7)
    s = f.report_settings
    assert s["every"] == 2 and s["columns"].tolist() == [1, 1, 0, 0] and s["sensor_columns"] is None and s["state_sigma"].dtype == np.float32 and s["seed"] == 7 and s["draws"] == 0
    for kw, msg in ((dict(every=-1), "every"), (dict(columns=[4]), "columns"), (dict(sensor_columns=[3]), "sensor_columns"), (dict(state_sigma=-1.0), "state_sigma"),
                    (dict(sensor_sigma=[1.0, 2.0]), "sensor_sigma"), (dict(seed=-1), "seed")):
        with pytest.raises(ValueError, match=msg):
            f.reports(**kw)
    assert f.report_settings["every"] == 2  # a refused call changes nothing
    with pytest.raises(ValueError, match="plan_delay = 4"):
        f.advance([_spline("zero", 0.0, 4, 1, b) for b in range(3)], 4, plan_delay=4)
    with pytest.raises(ValueError, match="3 splines of 2 controls"):
        f.advance([_spline("zero", 0.0, 4, 2, b) for b in range(3)], 4)
    with pytest.raises(ValueError, match="W must be"):
        f.advance_knots(np.ones((2, 4, 3)), np.ones((2, 3, 1)))


def test_spot_is_refused_by_name():
    from judo_amd.simulation import ClosedLoop, GpuSimulation, PlantFleet

    SpotPlantSet = type("SpotPlantSet", (), {})
    with pytest.raises(ValueError, match="Spot plant is not simulated here.*policy state.*warm start"):
        PlantFleet(SpotPlantSet(), [0], np.zeros(4))
    spot_task = SimpleNamespace(uses_locomotion_policy=True, reset=lambda: None)
    with pytest.raises(ValueError, match="Spot plant is not simulated here"):
        GpuSimulation(spot_task)
    with pytest.raises(ValueError, match="Spot plant is not simulated here"):
        ClosedLoop([SimpleNamespace(task=spot_task)], _Plants(1))
    with pytest.raises(ValueError, match="not found in task registry"):
        GpuSimulation("no_such_task")


# ---- GpuSimulation on a stand-in plant -----------------------------------------------------------------------------------------------------------------------------
class _OnePlant:
    """x <- x + sum(u) per step."""

    def __init__(self, log):
        self.log, self.x = log, None

    def set_state(self, x, time=None):
        self.x = np.array(x, dtype=np.float32).reshape(1, -1)

    def advance_knots(self, W, knots, steps=None, old=None):
        assert W.shape == (1, 1, 1) and W[0, 0, 0] == 1.0 and knots.shape[:2] == (1, 1)
        self.log.append(("physics", knots[0, 0].tolist()))
        self.x = self.x + knots.sum()

    def x_host(self):
        return self.x


def test_gpu_simulation_hook_order_and_pause():
    from judo_amd.simulation import GpuSimulation
    from judo_amd.structs import MujocoState
    from judo_amd.tasks import Cartpole

    log = []

    class Logged(Cartpole):
        def task_to_sim_ctrl(self, controls):
            log.append("task_to_sim_ctrl")
            return 2.0 * np.asarray(controls)

        def pre_sim_step(self):
            log.append("pre_sim_step")

        def post_sim_step(self):
            log.append(("post_sim_step", self.data.qpos.tolist(), self.data.time))

        def get_sim_metadata(self):
            return {"k": 1}

    sim = GpuSimulation(Logged(), plants=_OnePlant(log))
    assert sim.timestep == sim.task.dt and not sim.paused
    sim.task.data.qpos, sim.task.data.qvel, sim.task.data.time = np.array([1.0, 2.0]), np.array([3.0, 4.0]), 0.5
    sim.step([0.25])
    assert log == ["task_to_sim_ctrl", "pre_sim_step", ("physics", [0.5]), ("post_sim_step", [1.5, 2.5], 0.5 + sim.timestep)]  # task.data is updated before post_sim_step
    st = sim.sim_state
    assert isinstance(st, MujocoState) and st.qpos.tolist() == [1.5, 2.5] and st.qvel.tolist() == [3.5, 4.5] and st.time == 0.5 + sim.timestep and st.sim_metadata == {"k": 1}
    sim.pause()
    del log[:]
    sim.step([0.25])
    assert sim.paused and log == [] and sim.sim_state.qpos.tolist() == [1.5, 2.5]  # a no-op while paused
    sim.pause()
    sim.task.data.qpos = np.array([0.0, 0.0])  # what task.reset() does: the state lives in task.data
    sim.step([0.5])
    assert not sim.paused and sim.sim_state.qpos.tolist() == [1.0, 1.0]
    with pytest.raises(ValueError, match="nu = 1"):
        sim.step([0.1, 0.2])


# ---- ClosedLoop on stand-ins ---------------------------------------------------------------------------------------------------------------------------------------
class _Plants:
    """B stand-in plants of nx = 2 (nq = 1), nu = 1: x <- x + u per step, the control a constant the controller's spline names."""

    def __init__(self, B, dt=0.01, every=1):
        self.B, self.dt, self.nq = B, dt, 1
        self.x = np.zeros((B, 2), dtype=np.float32)
        self.steps_taken = np.zeros(B, dtype=np.int64)
        self.calls = []
        self.report_settings = {"every": every}
        self.states = self.sensors = self.controls = self.reported_states = self.reported_sensors = None

    def __len__(self):
        return self.B

    @property
    def time(self):
        return self.steps_taken * self.dt

    def x_host(self):
        return self.x.copy()

    def advance(self, splines, steps, plan_delay=0, old_splines=None):
        self.calls.append((steps, plan_delay, None if old_splines is None else [s.x[0, 0] for s in old_splines]))
        u = np.array([c.spline_data.x[0, 0] for c in splines], dtype=np.float32)
        self.controls = np.broadcast_to(u[:, None, None], (self.B, steps, 1)).copy()
        self.states = self.x[:, None, :] + np.cumsum(np.broadcast_to(u[:, None, None], (self.B, steps, 2)), axis=1)
        self.x = self.states[:, -1].copy()
        self.reported_states = self.states.copy()
        self.reported_states[:, 0::2] = np.nan
        self.steps_taken = self.steps_taken + steps


class _Ctrl:
    def __init__(self, u, log, freq=20.0):
        from judo_amd.structs import SplineData

        self.u, self.log, self.plans = u, log, 0
        self.controller_cfg = SimpleNamespace(control_freq=freq)
        self.task = SimpleNamespace(uses_locomotion_policy=False, reward=lambda states, sensors, controls, meta=None: np.array([float(np.asarray(states)[0, :, 0].sum())]))
        self.spline_data = SplineData([0.0, 1.0], [[0.0], [0.0]], "zero")
        self.system_metadata = {}

    def update_states(self, qpos, qvel, time, meta=None):
        self.log.append(("update_states", self.u, qpos.tolist(), qvel.tolist(), round(time, 9)))

    def update_action(self):
        from judo_amd.structs import SplineData

        self.plans += 1
        self.log.append(("plan", self.u))
        self.spline_data = SplineData([0.0, 1.0], [[self.u * self.plans], [self.u * self.plans]], "zero")


def test_closed_loop_on_stand_ins():
    from judo_amd.simulation import ClosedLoop

    log = []
    ctrls, plants = [_Ctrl(1.0, log), _Ctrl(2.0, log)], _Plants(2)
    loop = ClosedLoop(ctrls, plants)
    assert loop.steps_per_plan == 5 and loop.plan_delay == 0  # round(1 / (20 Hz * 0.01 s))
    assert ClosedLoop(ctrls, _Plants(2, dt=0.2)).steps_per_plan == 1  # at least 1
    loop = ClosedLoop(ctrls, plants, steps_per_plan=2, plan_delay=1)
    ret = loop.run(2)
    # one period: update_states on each member with its plant's state and clock, then the plans, then ONE advance with the old splines for the delay
    assert log[:4] == [("update_states", 1.0, [0.0], [0.0], 0.0), ("update_states", 2.0, [0.0], [0.0], 0.0), ("plan", 1.0), ("plan", 2.0)]
    assert log[4][:2] == ("update_states", 1.0) and log[4][2:] == ([2.0], [2.0], 0.02) and log[5][2:] == ([4.0], [4.0], 0.02)
    assert plants.calls == [(2, 1, [0.0, 0.0]), (2, 1, [1.0, 2.0])]
    # the realised rewards: the stand-in reward is the sum of the segment's positions -- plant 0: (1 + 2) + (4 + 6), plant 1: (2 + 4) + (8 + 12)
    assert ret is loop.returns and ret.tolist() == [13.0, 26.0] and len(loop.plan_ms) == 2 and loop.periods == 2
    states, controls = loop.trajectory()
    assert states.shape == (2, 4, 2) and controls.shape == (2, 4, 1) and states[0, :, 0].tolist() == [1.0, 2.0, 4.0, 6.0] and controls[1, :, 0].tolist() == [2.0, 2.0, 4.0, 4.0]

    # a fleet plans with its own update_action, once
    fleet_log = []
    fleet = SimpleNamespace(controllers=[_Ctrl(1.0, fleet_log), _Ctrl(2.0, fleet_log)], update_action=lambda: fleet_log.append("fleet plan"))
    ClosedLoop(fleet, _Plants(2), steps_per_plan=3).run(1)
    assert [e for e in fleet_log if not isinstance(e, tuple)] == ["fleet plan"]

    # estimators: windows of the estimator's horizon from the exact start state, the controls and the reports; a window may span two segments
    seen = []
    est = SimpleNamespace(horizon=3, weight_sens=None, observe=lambda x0, u, y: seen.append((x0.tolist(), u[:, 0].tolist(), y[:, 0].tolist())))
    after = []
    ClosedLoop([_Ctrl(1.0, [])], _Plants(1), steps_per_plan=2, estimators=[est], after_period=lambda lp, p: after.append((p, lp.periods))).run(3)
    assert len(seen) == 2 and after == [(0, 1), (1, 2), (2, 3)]
    assert seen[0][0] == [0.0, 0.0] and seen[0][1] == [1.0, 1.0, 2.0] and np.isnan(seen[0][2][0]) and seen[0][2][1] == 2.0 and np.isnan(seen[0][2][2])
    assert seen[1][0] == [4.0, 4.0] and seen[1][1] == [2.0, 3.0, 3.0]  # the second window starts inside the second segment, at the exact state

    for kw, msg in ((dict(controllers=ctrls[:1]), "1 controllers for B = 2"), (dict(steps_per_plan=0), "steps_per_plan = 0"), (dict(steps_per_plan=2, plan_delay=2), "plan_delay = 2"),
                    (dict(plan_delay=-1), "plan_delay = -1"), (dict(estimators=[est]), "1 estimators for B = 2")):
        args = dict(controllers=ctrls, plants=_Plants(2))
        args.update(kw)
        with pytest.raises(ValueError, match=msg):
            ClosedLoop(**args)
    with pytest.raises(ValueError, match="report nothing"):
        ClosedLoop(ctrls, _Plants(2, every=0), estimators=[est, None])
    with pytest.raises(RuntimeError, match="record=True"):
        ClosedLoop(ctrls, _Plants(2), record=False).trajectory()
