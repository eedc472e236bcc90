"""The plant side of the closed loop: B simulated plants advance on their controllers' plans in ONE call (`jh_plants_advance`, include/judo_amd.h).

The reference is a loop of two nodes: its `SimulationNode` evaluates the controller's spline at the plant's own clock and steps the plant once per model timestep
(judo/app/dora/simulation.py:52-82, judo/simulation/mj_simulation.py:33-46).  Here

  `GpuSimulation`  has the surface of `judo.simulation.MJSimulation` for one plant: `step(command)`, `sim_state`, `timestep`, `pause()`, `set_task()`, `task.reset()`;
  `PlantFleet`     holds B device-resident plants, members of a `GpuModelSet`; `advance(splines, steps)` is one `jh_plants_advance` call -- the B splines at the plants'
                   own clocks, one materialise launch on plants with a block per plant, and what each robot reports of the segment;
  `ClosedLoop`     runs controllers (a list, or any fleet with its one-launch `update_action`) against a `PlantFleet`, feeds estimators, and sums the realised rewards.

`plant_controls_host` and `plant_reports_host` restate the two kernels in numpy fp32, operation for operation: the device results equal them bit for bit
(tests/test_gpu_plant_controls.py, tests/test_gpu_plants_advance.py).

A deviation to know: the leap and fr3 kernels start their contact solver cold at the top of a launch, so a plant carries the solver's warm
start within a segment and not across segments; a MuJoCo plant carries `qacc_warmstart` from step to step.  One `advance(2 S)` and two `advance(S)` therefore differ in
contact by the solver's tolerance.  Spot plants (a policy state and a warm start per plant) are refused by name."""

from __future__ import annotations

import ctypes as C
import time as _time
from typing import Sequence

import numpy as np

from judo_amd import _lib
from judo_amd.spline import spline_weights
from judo_amd.structs import MujocoState, SplineData

MAX_FLEET_PLANT_BLOCKS = _lib.MAX_FLEET_PLANT_BLOCKS
MAX_KNOT_DIM = _lib.MAX_KNOT_DIM


# ---- the kernels' arithmetic, restated ---------------------------------------------------------------------------------------------------------------------------
def _order_key(a: np.ndarray) -> np.ndarray:
    """uint32 keys with key(a) < key(b) exactly when a < b as floats, -0.0 below +0.0 (k_plant_controls' clip compares these)."""
    b = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
    return np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000))


def plant_controls_host(W, knots, ctrl_lo_hi=None) -> np.ndarray:
    """`jh_plant_controls`, bit for bit: controls[b, s, u] = sum_k W[b, s, k] * knots[b, k, u] in fp32, acc = W[..., 0] * knots[:, 0], then acc = acc + W[..., k] *
    knots[:, k] with k ascending, every product and sum rounded on its own; then, with `ctrl_lo_hi` (nu lower bounds, then nu upper bounds), acc < lo -> lo and
    acc > hi -> hi in the order of the bits (-0.0 below +0.0), a NaN passing through.  `W` (B, S, K) or (S, K), `knots` (B, K, nu) or (K, nu); returns (B, S, nu) fp32."""
    W, kn = np.asarray(W, dtype=np.float32), np.asarray(knots, dtype=np.float32)
    W, kn = (W[None] if W.ndim == 2 else W), (kn[None] if kn.ndim == 2 else kn)
    if W.ndim != 3 or kn.ndim != 3 or W.shape[0] != kn.shape[0] or W.shape[2] != kn.shape[1]:
        raise ValueError(f"W must be (B, S, K) and knots (B, K, nu), got {W.shape} and {kn.shape}")
    B, S, K = W.shape
    nu = kn.shape[2]
    if min(B, S, K, nu) < 1 or K * nu > MAX_KNOT_DIM:
        raise ValueError(f"W of shape {W.shape}, knots of shape {kn.shape}: B, S, K and nu must be at least 1 and K * nu at most {MAX_KNOT_DIM} (include/judo_amd.h JH_MAX_KNOT_DIM)")
    with np.errstate(over="ignore", invalid="ignore"):
        acc = W[:, :, 0, None] * kn[:, None, 0, :]
        for k in range(1, K):
            p = W[:, :, k, None] * kn[:, None, k, :]
            acc = acc + p
    assert acc.dtype == np.float32
    if ctrl_lo_hi is not None:
        lohi = np.asarray(ctrl_lo_hi, dtype=np.float32).reshape(-1)
        if lohi.shape != (2 * nu,):
            raise ValueError(f"ctrl_lo_hi must hold 2 * nu = {2 * nu} entries, the lower bounds and then the upper ones, got {lohi.shape}")
        lo, hi = np.broadcast_to(lohi[:nu], acc.shape), np.broadcast_to(lohi[nu:], acc.shape)
        ok = ~np.isnan(acc)
        acc = np.where(ok & (_order_key(acc) < _order_key(lo)), lo, acc)
        acc = np.where(ok & (_order_key(acc) > _order_key(hi)), hi, acc)
    return np.ascontiguousarray(acc, dtype=np.float32)


def reported_steps(count, steps: int, every: int) -> np.ndarray:
    """(B, steps) bools: step s of plant b is reported when (count[b] + s + 1) % every == 0, `count[b]` being the steps the plant has taken before the segment."""
    count = np.atleast_1d(np.asarray(count, dtype=np.int64))
    if int(every) != every or every < 1:
        raise ValueError(f"every = {every} must be at least 1")
    if (count < 0).any():
        raise ValueError(f"count = {count.tolist()} holds a negative number of steps")
    return (count[:, None] + np.arange(int(steps))[None, :] + 1) % int(every) == 0


def plant_reports_host(states, count, every: int = 1, columns=None, sigma=None, noise=None) -> tuple[np.ndarray, np.ndarray]:
    """`jh_plant_reports` on one of its two arrays, bit for bit: (reports (B, S, n) fp32, carry (B, n) fp32).  `states` (B, S, n) is what the segment wrote (the states,
    or the sensors); a report entry is states + sigma[j] * noise[b, s, j] -- the product, then the sum, each rounded to fp32; just the state where `sigma` or `noise`
    is None -- where step s of plant b is reported (`reported_steps`) and column j's entry of `columns` (n bools; None: all) is true, and NaN elsewhere.  The carry is
    states[:, -1], the exact state."""
    st = np.asarray(states, dtype=np.float32)
    if st.ndim != 3 or min(st.shape) < 1:
        raise ValueError(f"states must be (B, S, n) with no empty axis, got {st.shape}")
    B, S, n = st.shape
    steps = reported_steps(count, S, every)
    if steps.shape[0] != B:
        raise ValueError(f"count must hold B = {B} entries, got {steps.shape[0]}")
    cols = np.ones(n, dtype=bool) if columns is None else np.asarray(columns).astype(bool).reshape(-1)
    if cols.shape != (n,):
        raise ValueError(f"columns must hold n = {n} entries, got {cols.shape}")
    v = st
    if sigma is not None and noise is not None:
        sg, nz = np.asarray(sigma, dtype=np.float32).reshape(-1), np.asarray(noise, dtype=np.float32)
        if sg.shape != (n,) or nz.shape != st.shape:
            raise ValueError(f"sigma must be (n,) = ({n},) and noise {st.shape}, got {sg.shape} and {nz.shape}")
        with np.errstate(over="ignore", invalid="ignore"):
            p = sg * nz
            v = st + p
    out = np.where(steps[:, :, None] & cols[None, None, :], v, np.float32(np.nan)).astype(np.float32)
    return out, st[:, -1].copy()


# ---- the splines of a segment, without a device ------------------------------------------------------------------------------------------------------------------
def _spline_of(s) -> SplineData:
    """A `SplineData` record, or a controller's (`Controller.spline_data`)."""
    if isinstance(s, SplineData):
        return s
    if hasattr(s, "spline_data"):
        return s.spline_data
    raise ValueError(f"a spline must be a SplineData record or a controller with `spline_data`, got {type(s).__name__}")


def _members(splines) -> list:
    """A list of splines or controllers, or a fleet's controllers."""
    return list(splines.controllers) if hasattr(splines, "controllers") else list(splines)


def spline_rows(splines, times, dt: float, first: int, last: int) -> tuple[np.ndarray, np.ndarray]:
    """(W (B, last - first, K) fp32, knots (B, K, nu) fp32): plant b's spline at its own clock, steps first .. last - 1 of a segment that starts at `times[b]` -- the
    queries are times[b] + dt * s.  Every spline has the same K and nu (their kinds and knot times are their own).  What `PlantFleet.advance` uploads."""
    recs = [_spline_of(s) for s in _members(splines)]
    times = np.atleast_1d(np.asarray(times, dtype=np.float64))
    if len(recs) != len(times):
        raise ValueError(f"{len(recs)} splines for B = {len(times)} plants")
    shapes = {r.x.shape for r in recs}
    if len(shapes) != 1 or len(next(iter(shapes))) != 2:
        raise ValueError(f"every plant's spline must have knots of one shape (K, nu), got {sorted(shapes)}")
    K, nu = recs[0].x.shape
    if K * nu > MAX_KNOT_DIM:
        raise ValueError(f"K * nu = {K} * {nu} exceeds {MAX_KNOT_DIM} (include/judo_amd.h JH_MAX_KNOT_DIM)")
    W = np.stack([spline_weights(r.kind, r.t, times[b] + dt * np.arange(first, last)) for b, r in enumerate(recs)]).astype(np.float32)
    return W, np.stack([r.x for r in recs]).astype(np.float32)


def segment_rows(splines, old_splines, times, dt: float, steps: int, plan_delay: int):
    """The two control ranges of a segment of `steps` steps: (old, new), each (W, knots) as `spline_rows` gives them, `old` None without a delay.  With
    `plan_delay` = L > 0 steps 0 .. L - 1 follow `old_splines` and steps L .. steps - 1 the new ones: a plan takes effect L steps after the state it was planned from."""
    steps, L = int(steps), int(plan_delay)
    if steps < 1:
        raise ValueError(f"steps = {steps} must be at least 1")
    if not 0 <= L < steps:
        raise ValueError(f"plan_delay = {plan_delay} outside [0, steps = {steps}): a plan must take effect within its own segment")
    if L > 0 and old_splines is None:
        raise ValueError(f"plan_delay = {L} needs old_splines: the plans the plants follow until the new ones take effect")
    old = spline_rows(old_splines, times, dt, 0, L) if L > 0 else None
    return old, spline_rows(splines, times, dt, L, steps)


def _refuse_spot(what) -> None:
    if type(what).__name__ == "SpotPlantSet" or getattr(getattr(what, "task", None), "uses_locomotion_policy", False):
        raise ValueError("a Spot plant is not simulated here: the Spot policy simulation carries policy state (the policy outputs) and the solver's warm start from step "
                         "to step, which jh_plants_advance does not carry; PlantFleet and GpuSimulation take the closed-form families, the leap family and fr3_pick")


# ---- B plants on the device ----------------------------------------------------------------------------------------------------------------------------------------
class PlantFleet:
    """B device-resident plants, plant b a member `truth[b]` of a `GpuModelSet` (cartpole, cylinder_push, the leap family, or an fr3_pick set).

        fleet = PlantFleet(model_set, truth=[2, 0, 2], x0=x0)        # x0 (B, nx), or (nx,) for every plant
        fleet.reports(every=2, columns=range(nq), state_sigma=1e-3)   # optional: what a robot reports of every segment
        fleet.advance(controllers, steps=4)                            # ONE jh_plants_advance call
        fleet.states, fleet.sensors, fleet.controls                    # (B, steps, .) device tensors of the last segment; fleet.x (B, nx), fleet.time, fleet.steps_taken
        fleet.reported_states, fleet.reported_sensors                  # NaN where nothing was reported

    Rows b of `states` and `sensors` are bit for bit what `jh_rollout_materialize` writes on plant `truth[b]`'s own model from `x[b]` with the segment's controls.
    `ctrl_lo_hi` (2 * nu: lower bounds, then upper ones) clips the evaluated controls; the kernels apply the model's own control range either way."""

    def __init__(self, model_set, truth: Sequence[int], x0, ctrl_lo_hi=None, time: float = 0.0) -> None:
        _refuse_spot(model_set)
        if not hasattr(model_set, "models") or len(model_set.models) < 1:
            raise ValueError(f"model_set must be a GpuModelSet, got {type(model_set).__name__}")
        from judo_amd.rollout_backend import check_plant_table

        first = model_set.models[0]
        self.model_set, self.models = model_set, model_set.models
        self.truth = check_plant_table(truth, len(model_set.models))
        self.B, self.nq, self.nx, self.nu, self.ns, self.dt = len(self.truth), int(first.nq), int(first.nx), int(first.nu), int(first.ns), float(first.dt)
        self._lohi_host = None
        if ctrl_lo_hi is not None:
            self._lohi_host = np.asarray(ctrl_lo_hi, dtype=np.float32).reshape(-1)
            if self._lohi_host.shape != (2 * self.nu,) or np.isnan(self._lohi_host).any():
                raise ValueError(f"ctrl_lo_hi must hold 2 * nu = {2 * self.nu} numbers, the lower bounds and then the upper ones, got {ctrl_lo_hi!r}")
        self._x0 = self._checked_x(x0)
        self._time0 = float(time)
        self.steps_taken = np.zeros(self.B, dtype=np.int64)
        self._every, self._columns, self._sensor_columns, self._state_sigma, self._sensor_sigma, self._seed, self._draw = 0, None, None, None, None, 0, 0
        self.device = first.device
        self.x = self._to_device(self._x0)
        self._lohi = None if self._lohi_host is None else self._to_device(self._lohi_host)
        self._truth_c = (C.c_int * self.B)(*self.truth)
        self._seg: dict = {}  # the segment buffers by S
        self.states = self.sensors = self.controls = self.reported_states = self.reported_sensors = None
        self.last_noise = self.last_sensor_noise = None  # the standard normals the last segment's reports were drawn with, (B, S, nx) and (B, S, ns)
        self._report_dev: dict = {}

    # ---- host-side checks ------------------------------------------------------------------------------------------------------------------------------------
    def _checked_x(self, x) -> np.ndarray:
        x = np.asarray(x, dtype=np.float32)
        if x.shape == (self.nx,):
            x = np.tile(x, (self.B, 1))
        if x.shape != (self.B, self.nx) or not np.isfinite(x).all():
            raise ValueError(f"x0 must be finite and (B, nx) = ({self.B}, {self.nx}) or (nx,), got shape {x.shape}")
        return np.ascontiguousarray(x)

    def _to_device(self, a: np.ndarray):
        import torch

        return torch.from_numpy(np.ascontiguousarray(a)).to(self.device)

    # ---- state ---------------------------------------------------------------------------------------------------------------------------------------------------
    def __len__(self) -> int:
        return self.B

    @property
    def time(self) -> np.ndarray:
        """(B,) fp64: every plant's own clock, the start time plus steps_taken * dt."""
        return self._time0 + self.steps_taken * self.dt

    def x_host(self) -> np.ndarray:
        """One download of `x`, (B, nx) fp32."""
        return self.x.cpu().numpy()

    def set_state(self, x, time: float | None = None) -> None:
        """Put the plants at `x` ((B, nx) or (nx,)): an upload.  `time` restarts the clocks there."""
        self.x.copy_(self._to_device(self._checked_x(x)))
        if time is not None:
            self._time0, self.steps_taken = float(time), np.zeros(self.B, dtype=np.int64)

    def reports(self, every: int = 1, columns=None, state_sigma=None, sensor_sigma=None, seed: int = 0, sensor_columns=None) -> None:
        """What `advance` also writes to `reported_states` and `reported_sensors` from now on: every `every`-th step of a plant's own count (the stride carries across
        segments), the state columns `columns` (indices; None: all) and the sensor columns `sensor_columns`, each entry plus `state_sigma` / `sensor_sigma` (a
        non-negative scalar or a vector; None: no noise) times a standard normal drawn with `jh_noise_normal` under `seed`, a fresh draw per segment.  `every = 0`
        turns the reports off."""
        if int(every) != every or every < 0:
            raise ValueError(f"every = {every} must be at least 1 (0 turns the reports off)")

        def mask(cols, n, name):
            if cols is None:
                return None
            idx = [int(c) for c in cols]
            if any(not 0 <= c < n for c in idx):
                raise ValueError(f"{name} = {list(cols)!r} names a column outside [0, {n})")
            m = np.zeros(n, dtype=np.uint8)
            m[idx] = 1
            return m

        def sig(s, n, name):
            if s is None:
                return None
            v = np.asarray(s, dtype=np.float64)
            v = np.full(n, float(v)) if v.ndim == 0 else v
            if v.shape != (n,) or not np.isfinite(v).all() or (v < 0).any():
                raise ValueError(f"{name} must be a non-negative, finite scalar or ({n},) vector, got {s!r}")
            return v.astype(np.float32)

        cols, scols = mask(columns, self.nx, "columns"), mask(sensor_columns, self.ns, "sensor_columns")
        ss, es = sig(state_sigma, self.nx, "state_sigma"), sig(sensor_sigma, self.ns, "sensor_sigma")
        if int(seed) != seed or seed < 0:
            raise ValueError(f"seed = {seed!r} must be a non-negative integer")
        self._every, self._columns, self._sensor_columns, self._state_sigma, self._sensor_sigma, self._seed, self._draw = int(every), cols, scols, ss, es, int(seed), 0
        self._report_dev = {k: self._to_device(v) for k, v in (("columns", cols), ("sensor_columns", scols), ("state_sigma", ss), ("sensor_sigma", es)) if v is not None}
        if not self._every:
            self.reported_states = self.reported_sensors = None

    @property
    def report_settings(self) -> dict:
        """What `reports` set: every, the column masks (uint8 or None), the sigmas (fp32 or None), the seed and the number of draws taken."""
        return dict(every=self._every, columns=self._columns, sensor_columns=self._sensor_columns, state_sigma=self._state_sigma, sensor_sigma=self._sensor_sigma,
                    seed=self._seed, draws=self._draw)

    # ---- the segment -----------------------------------------------------------------------------------------------------------------------------------------------
    def _segment(self, S: int) -> dict:
        import torch

        seg = self._seg.get(S)
        if seg is None:
            def buf(n):
                return torch.empty((self.B, S, n), dtype=torch.float32, device=self.device)

            seg = self._seg[S] = dict(states=buf(self.nx), sensors=buf(self.ns), controls=buf(self.nu), reported_states=buf(self.nx), reported_sensors=buf(self.ns),
                                      noise=buf(self.nx), noise_sens=buf(self.ns))
        return seg

    def advance(self, splines, steps: int, plan_delay: int = 0, old_splines=None) -> None:
        """Every plant advances `steps` physics steps on its spline (`SplineData` records, controllers, or a fleet of controllers), evaluated at its own clock: one
        `jh_plants_advance` call.  With `plan_delay` = L > 0 the first L steps follow `old_splines` (one more `jh_plant_controls` launch into the same controls buffer)."""
        old, new = segment_rows(splines, old_splines, self.time, self.dt, steps, plan_delay)
        if new[1].shape[0] != self.B or new[1].shape[2] != self.nu:
            raise ValueError(f"{new[1].shape[0]} splines of {new[1].shape[2]} controls for B = {self.B} plants of nu = {self.nu}")
        self.advance_knots(new[0], new[1], steps=int(steps), old=old)

    def advance_knots(self, W, knots, steps: int | None = None, old=None) -> None:
        """`advance` on the weight rows themselves: `W` (B, steps - L, K) and `knots` (B, K, nu) fill steps L .. steps - 1, `old` = (W (B, L, K'), knots (B, K', nu)) the
        L steps in front of them."""
        from judo_amd.device import current_stream_ptr

        lib = _lib.lib()
        W, knots = np.ascontiguousarray(W, dtype=np.float32), np.ascontiguousarray(knots, dtype=np.float32)
        if W.ndim != 3 or knots.ndim != 3 or W.shape[0] != self.B or knots.shape[0] != self.B or W.shape[2] != knots.shape[1] or knots.shape[2] != self.nu:
            raise ValueError(f"W must be (B, steps, K) and knots (B, K, nu) with B = {self.B}, nu = {self.nu}, got {W.shape} and {knots.shape}")
        L = 0 if old is None else int(np.asarray(old[0]).shape[1])
        S = W.shape[1] + L if steps is None else int(steps)
        if S != W.shape[1] + L:
            raise ValueError(f"steps = {S}, but W holds {W.shape[1]} rows per plant behind {L} delayed ones")
        seg, stream = self._segment(S), current_stream_ptr()
        if L:
            Wo, ko = self._to_device(np.ascontiguousarray(old[0], dtype=np.float32)), self._to_device(np.ascontiguousarray(old[1], dtype=np.float32))
            _lib.check(lib.jh_plant_controls(_lib.ptr(Wo), _lib.ptr(ko), int(ko.shape[1] * ko.shape[2]), _lib.ptr(self._lohi), self.B, L, int(ko.shape[1]), self.nu, 0, S,
                                             _lib.ptr(seg["controls"]), stream), "jh_plant_controls")
        W_d, k_d = self._to_device(W), self._to_device(knots)
        rep, dev = self._every > 0, self._report_dev
        noise = noise_sens = None
        if rep and self._state_sigma is not None:
            noise = seg["noise"]
            _lib.check(lib.jh_noise_normal(self._seed, self._draw, self.B * S, 0, self.nx, _lib.ptr(noise), self.nx, stream), "jh_noise_normal")
            self._draw += 1
        if rep and self._sensor_sigma is not None and self.ns:
            noise_sens = seg["noise_sens"]
            _lib.check(lib.jh_noise_normal(self._seed, self._draw, self.B * S, 0, self.ns, _lib.ptr(noise_sens), self.ns, stream), "jh_noise_normal")
            self._draw += 1
        count = (C.c_int * self.B)(*[int(c) for c in self.steps_taken])
        st = lib.jh_plants_advance(self.model_set.handle, self._truth_c, self.B, _lib.ptr(self.x), _lib.ptr(W_d), _lib.ptr(k_d), int(knots.shape[1] * knots.shape[2]),
                                   int(knots.shape[1]), _lib.ptr(self._lohi), L, S, _lib.ptr(seg["controls"]), _lib.ptr(seg["states"]),
                                   _lib.ptr(seg["sensors"]) if self.ns else None, count, max(self._every, 1), _lib.ptr(noise), _lib.ptr(dev.get("state_sigma")),
                                   _lib.ptr(dev.get("columns")), _lib.ptr(seg["reported_states"]) if rep else None, _lib.ptr(noise_sens), _lib.ptr(dev.get("sensor_sigma")),
                                   _lib.ptr(dev.get("sensor_columns")), _lib.ptr(seg["reported_sensors"]) if rep and self.ns else None, stream)
        _lib.check(st, "jh_plants_advance")
        self.steps_taken = self.steps_taken + S
        self.states, self.sensors, self.controls = seg["states"], seg["sensors"], seg["controls"]
        self.reported_states = seg["reported_states"] if rep else None
        self.reported_sensors = seg["reported_sensors"] if rep and self.ns else None
        self.last_noise, self.last_sensor_noise = noise, noise_sens


# ---- one plant with the reference's surface ----------------------------------------------------------------------------------------------------------------------
class GpuSimulation:
    """`judo.simulation.MJSimulation` on the device (judo/simulation/mj_simulation.py:20-60): `step(command)`, `sim_state`, `timestep`, `pause()`, `set_task()`.  The
    state lives in `task.data`, as the reference's lives in the task's MjData: `task.reset()` moves the plant, and a step reads `task.data`, takes one physics step on
    the device (B = 1, S = 1 of `jh_plants_advance`) and writes `task.data.qpos`, `qvel` and `time` back.  `description` makes the plant differ from the task's own
    model (`models.scaled_description`): the controller plans on the nominal one, the simulation steps the true one."""

    def __init__(self, init_task: str = "cylinder_push", description: dict | None = None, plants=None) -> None:
        self._description, self._given_plants = description, plants
        self.paused = False
        self.set_task(init_task)

    def set_task(self, task_name) -> None:
        """judo/simulation/base.py:30-38: a registered task by name (or a task instance), reset."""
        from judo_amd.tasks import get_registered_tasks

        if isinstance(task_name, str):
            entry = get_registered_tasks().get(task_name)
            if entry is None:
                raise ValueError(f"Init task {task_name} not found in task registry")
            task = entry[0]()
        else:
            task = task_name
        _refuse_spot(type("_", (), {"task": task})())
        self.task = task
        self.task.reset()
        self._plants = self._given_plants  # made at the first step: the device is not touched before

    def _make_plants(self):
        from judo_amd.device import GpuModel, GpuModelSet

        model = GpuModel(self._description, None) if self._description is not None else self.task.gpu_model()
        return PlantFleet(GpuModelSet([model]), [0], np.concatenate([self.task.data.qpos, self.task.data.qvel]))

    @property
    def timestep(self) -> float:
        return self.task.dt

    def pause(self) -> None:
        """judo/simulation/base.py:40-42: toggles."""
        self.paused = not self.paused

    def step(self, command) -> None:
        """judo/simulation/mj_simulation.py:33-46: no-op while paused; else task_to_sim_ctrl, pre_sim_step, one physics step, task.data, post_sim_step."""
        if self.paused:
            return
        task = self.task
        ctrl = np.asarray(task.task_to_sim_ctrl(np.asarray(command, dtype=np.float64)), dtype=np.float32).reshape(-1)
        if ctrl.shape != (task.nu,):
            raise ValueError(f"command must hold nu = {task.nu} controls, got shape {np.shape(command)}")
        task.pre_sim_step()
        if self._plants is None:
            self._plants = self._make_plants()
        p = self._plants
        p.set_state(np.concatenate([task.data.qpos, task.data.qvel]).astype(np.float32))
        p.advance_knots(np.ones((1, 1, 1), dtype=np.float32), ctrl[None, None, :])  # (1.0 * command is the command)
        x = np.asarray(p.x_host(), dtype=np.float64)[0]
        task.data.qpos, task.data.qvel = x[: task.nq].copy(), x[task.nq :].copy()
        task.data.time = task.data.time + self.timestep
        task.post_sim_step()

    @property
    def sim_state(self) -> MujocoState:
        d = self.task.data
        return MujocoState(time=float(d.time), qpos=np.array(d.qpos, dtype=np.float64), qvel=np.array(d.qvel, dtype=np.float64), sim_metadata=self.task.get_sim_metadata())


# ---- the loop ----------------------------------------------------------------------------------------------------------------------------------------------------
def _host(a) -> np.ndarray:
    return a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)


class ClosedLoop:
    """Controllers against plants, one control period at a time.

        loop = ClosedLoop(fleet_of_controllers, plants, steps_per_plan=4, estimators=[ReportEstimator(...), ...])
        loop.run(10); loop.returns, loop.plan_ms, loop.trajectory()

    `controllers`: a list of controllers (each plans with its own `update_action`), or any fleet -- `ControllerFleet`, the ensemble, randomised, weighted and fr3 fleets --
    which plans with its one-launch `update_action`.  One period: one download of `x`; `update_states` on each member with its plant's state and clock; plan; `advance`;
    each plant's segment handed to its estimator in windows of the estimator's horizon, `observe(x0, controls, reported_states[, reported_sensors])`; each plant's
    realised reward of the segment (`Task.reward`, which is `jh_task_reward` with that member's task parameters and phase) added to `returns[b]`.
    `after_period(loop, period)`, if given, runs behind each period: where an estimator's belief is handed to its controller (`est.update(); est.apply_risk(ctrl)`)."""

    def __init__(self, controllers, plants, steps_per_plan: int | None = None, plan_delay: int = 0, estimators=None, after_period=None, record: bool = True) -> None:
        self.fleet = controllers if hasattr(controllers, "controllers") and hasattr(controllers, "update_action") else None
        self.controllers = _members(controllers)
        self.plants = plants
        B = len(plants)
        if len(self.controllers) != B:
            raise ValueError(f"{len(self.controllers)} controllers for B = {B} plants")
        for c in self.controllers:
            _refuse_spot(c)
        if steps_per_plan is None:
            steps_per_plan = max(1, int(round(1.0 / (self.controllers[0].controller_cfg.control_freq * plants.dt))))
        if int(steps_per_plan) != steps_per_plan or steps_per_plan < 1:
            raise ValueError(f"steps_per_plan = {steps_per_plan} must be at least 1")
        self.steps_per_plan = int(steps_per_plan)
        if int(plan_delay) != plan_delay or not 0 <= plan_delay < self.steps_per_plan:
            raise ValueError(f"plan_delay = {plan_delay} outside [0, steps_per_plan = {self.steps_per_plan})")
        self.plan_delay = int(plan_delay)
        self.estimators = None if estimators is None else list(estimators)
        if self.estimators is not None:
            if len(self.estimators) != B:
                raise ValueError(f"{len(self.estimators)} estimators for B = {B} plants (None for a plant without one)")
            if any(e is not None for e in self.estimators) and getattr(plants, "report_settings", {"every": 1})["every"] < 1:
                raise ValueError("estimators are given, but the plants report nothing: call plants.reports(...) first")
        self._pending = [None] * B  # the window an estimator's plant is filling: dict(x0, controls, states, sensors)
        self.after_period, self.record = after_period, bool(record)
        self.returns = np.zeros(B, dtype=np.float64)
        self.plan_ms: list[float] = []
        self.periods = 0
        self._traj: list[tuple] = []

    def _plan(self) -> None:
        if self.fleet is not None:
            self.fleet.update_action()
        else:
            for c in self.controllers:
                c.update_action()

    def _hand_over(self, b: int, est, x0: np.ndarray, seg: dict) -> None:
        """Plant b's segment to its estimator, in windows of the estimator's horizon; a window may span segments."""
        want_sens = getattr(est, "weight_sens", None) is not None
        for s in range(seg["controls"].shape[1]):
            w = self._pending[b]
            if w is None:
                w = self._pending[b] = dict(x0=(x0[b] if s == 0 else seg["states"][b, s - 1]).copy(), controls=[], states=[], sensors=[])
            w["controls"].append(seg["controls"][b, s])
            w["states"].append(seg["reported_states"][b, s])
            if want_sens:
                w["sensors"].append(seg["reported_sensors"][b, s])
            if len(w["controls"]) == est.horizon:
                self._pending[b] = None
                args = (w["x0"], np.stack(w["controls"]), np.stack(w["states"]))
                est.observe(*args, np.stack(w["sensors"])) if want_sens else est.observe(*args)

    def run(self, periods: int) -> np.ndarray:
        """`periods` control periods; returns `returns`, (B,) fp64, the realised rewards summed so far."""
        p, S = self.plants, self.steps_per_plan
        for _ in range(int(periods)):
            x0 = np.asarray(p.x_host())
            t = np.asarray(p.time, dtype=np.float64)
            for b, c in enumerate(self.controllers):
                c.update_states(x0[b, : p.nq].astype(np.float64), x0[b, p.nq :].astype(np.float64), float(t[b]), getattr(c, "system_metadata", None))
            old = [c.spline_data for c in self.controllers] if self.plan_delay else None
            t0 = _time.perf_counter()
            self._plan()
            self.plan_ms.append(1e3 * (_time.perf_counter() - t0))
            p.advance(self.controllers, S, self.plan_delay, old)
            for b, c in enumerate(self.controllers):
                r = c.task.reward(p.states[b : b + 1], None if p.sensors is None else p.sensors[b : b + 1], p.controls[b : b + 1], getattr(c, "system_metadata", None))
                self.returns[b] += float(_host(r).reshape(-1)[0])
            seg = None
            if self.record or self.estimators is not None:
                seg = {k: None if getattr(p, k, None) is None else _host(getattr(p, k)) for k in ("states", "controls", "reported_states", "reported_sensors")}
            if self.estimators is not None:
                for b, est in enumerate(self.estimators):
                    if est is not None:
                        self._hand_over(b, est, x0, seg)
            if self.record:
                self._traj.append((seg["states"].copy(), seg["controls"].copy()))
            self.periods += 1
            if self.after_period is not None:
                self.after_period(self, self.periods - 1)
        return self.returns

    def trajectory(self) -> tuple[np.ndarray, np.ndarray]:
        """(states (B, periods * steps_per_plan, nx), controls (B, periods * steps_per_plan, nu)) of every recorded period, fp32."""
        if not self._traj:
            raise RuntimeError("trajectory() needs run() with record=True")
        return np.concatenate([s for s, _ in self._traj], axis=1), np.concatenate([u for _, u in self._traj], axis=1)


__all__ = ["ClosedLoop", "GpuSimulation", "MAX_FLEET_PLANT_BLOCKS", "PlantFleet", "plant_controls_host", "plant_reports_host", "reported_steps", "segment_rows", "spline_rows"]
