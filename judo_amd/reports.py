"""Identify the plant from a robot's reports: partial, sparse, and Spot (`jh_plant_residuals_reports`, include/judo_amd.h).

`identify.PlantEstimator` takes a full state after every physics step of the model.  A robot reports at its control rate, reports joint angles and an object pose rather
than velocities, and often reports sensor readings rather than states.  ONE rule covers all of it: an entry of an observation that is NaN was not reported and is no
evidence for or against any plant.  Whole step rows are NaN where the reports are slower than the model, the velocity columns are NaN where only positions arrive, a
dropped reading is a NaN.

`plant_residuals_reports_host` restates the kernel's arithmetic in numpy fp32, operation for operation; the device result equals it bit for bit
(tests/test_gpu_plant_residuals_reports.py).  `ReportEstimator` is `PlantEstimator` under that rule, with sensors as evidence, for a `GpuModelSet`;
`SpotReportEstimator` is the estimator of a `SpotPlantSet`, whose recorded window carries the policy state the Spot rollout needs.  Both share the ring buffer's
bookkeeping, the posterior arithmetic, `apply` and `apply_risk` with `PlantEstimator` (`identify.PlantBelief`).  The reference has no counterpart."""

from __future__ import annotations

import ctypes as C
from types import SimpleNamespace
from typing import Sequence

import numpy as np
import torch

from judo_amd import _lib
from judo_amd.identify import MAX_ID_HORIZON, MAX_ID_QUATS, PlantBelief, PlantEstimator, _host, check_quat_adr
from judo_amd.models import layout

MAX_FLEET_PLANT_BLOCKS = _lib.MAX_FLEET_PLANT_BLOCKS
POLICY_COMMAND_DIM, POLICY_OUTPUT_DIM = 25, 12


def plant_residuals_reports_host(pred, obs, weight, quat_adr: Sequence[int] = (), nq: int | None = None, pred_sens=None, obs_sens=None, weight_sens=None,
                                 window_major: bool = False) -> np.ndarray:
    """The weighted squared prediction error of every plant on every window over the REPORTED entries, (M, W) fp32.  `pred` (M * W, H, nx) holds plant m's prediction of
    window w in row m * W + w (plant-major, the plants launch of a `GpuModelSet`) or, with `window_major`, in row w * M + m (`jh_policy_rollout_plants` with a problem
    per window); `obs` (W, H, nx), NaN where nothing was reported; `weight` (nx); `quat_adr` inside [0, `nq`) (None: nx).  `pred_sens` (M * W, H, ns) in the order of
    `pred`, `obs_sens` (W, H, ns) and `weight_sens` (ns) add sensor evidence; all three or none.  What `jh_plant_residuals_reports` computes, bit for bit, every product
    and sum rounded to fp32 on its own: per step and quaternion dot = ((p0 * o0 + p1 * o1) + p2 * o2) + p3 * o3, and where dot < 0 -- never with a NaN among the four
    observed coordinates -- the prediction is compared against -o; per coordinate t = +0.0 where o is NaN, else e = p - o', t = (weight * e) * e; per step the t are
    added in ascending d, the sensor terms behind the state's; per window the H step sums are placed in 64 slots, the rest +0.0, and halved six times.  A NaN
    prediction under a reported entry gives NaN, under an unreported one nothing."""
    p, o, wt = np.asarray(pred, dtype=np.float32), np.asarray(obs, dtype=np.float32), np.asarray(weight, dtype=np.float32).reshape(-1)
    if o.ndim != 3:
        raise ValueError(f"obs must be (W, H, nx), got {o.shape}")
    W, H, nx = o.shape
    if W < 1 or nx < 1 or not 1 <= H <= MAX_ID_HORIZON:
        raise ValueError(f"obs of shape {o.shape}: W and nx must be at least 1 and H in [1, {MAX_ID_HORIZON}] (include/judo_amd.h JH_MAX_ID_HORIZON)")
    if p.ndim != 3 or p.shape[1:] != (H, nx) or p.shape[0] < W or p.shape[0] % W != 0:
        raise ValueError(f"pred must be (M * W, H, nx) = (M * {W}, {H}, {nx}), got {p.shape}")
    if wt.shape != (nx,):
        raise ValueError(f"weight must have nx = {nx} entries, got {wt.shape}")
    nq = nx if nq is None else int(nq)
    if not 0 <= nq <= nx:
        raise ValueError(f"nq = {nq} outside [0, nx = {nx}]")
    quats = check_quat_adr(quat_adr, nq)
    M = p.shape[0] // W
    given = [a is not None for a in (pred_sens, obs_sens, weight_sens)]
    if any(given) and not all(given):
        raise ValueError("pred_sens, obs_sens and weight_sens: all three or none")
    if all(given):
        ps, os_, ws = np.asarray(pred_sens, dtype=np.float32), np.asarray(obs_sens, dtype=np.float32), np.asarray(weight_sens, dtype=np.float32).reshape(-1)
        ns = ws.size
        if ns < 1 or os_.shape != (W, H, ns) or ps.shape != (M * W, H, ns):
            raise ValueError(f"sensors: weight_sens must have ns >= 1 entries, obs_sens be (W, H, ns) = ({W}, {H}, {ns}) and pred_sens (M * W, H, ns) = ({M * W}, {H}, {ns}), "
                             f"got {ws.shape}, {os_.shape} and {ps.shape}")
    else:
        ns = 0

    def by_plant(a):  # (M, W, H, n) whichever way the rows lie
        return a.reshape(W, M, H, a.shape[-1]).transpose(1, 0, 2, 3) if window_major else a.reshape(M, W, H, a.shape[-1])

    p = by_plant(p)
    oo = np.broadcast_to(o, p.shape).copy()
    with np.errstate(over="ignore", invalid="ignore"):
        for a in quats:
            dot = p[..., a] * o[..., a]
            for i in (1, 2, 3):
                dot = dot + p[..., a + i] * o[..., a + i]
            oo[..., a : a + 4] = np.where((dot < 0)[..., None], -o[..., a : a + 4], o[..., a : a + 4])  # (NaN < 0 is False: no flip)
        e = p - oo
        t = np.where(np.isnan(oo), np.float32(0), (wt * e) * e)  # (np.isnan is the bit test: exponent all ones, mantissa not zero)
        s = t[..., 0].copy()
        for d in range(1, nx):
            s = s + t[..., d]
        if ns:
            es = by_plant(ps) - os_
            ts = np.where(np.isnan(os_), np.float32(0), (ws * es) * es)
            for d in range(ns):
                s = s + ts[..., d]
        v = np.zeros((M, W, 64), dtype=np.float32)
        v[..., :H] = s
        for k in (32, 16, 8, 4, 2, 1):
            v[..., :k] = v[..., :k] + v[..., k : 2 * k]
    assert v.dtype == np.float32
    return v[..., 0].copy()


def _check_sigma(sigma, n: int, name: str) -> np.ndarray:
    """1 / sigma**2 as (n,) fp32 from a positive, finite scalar or (n,) vector (None: ones); raises ValueError naming it."""
    s = np.ones(n) if sigma is None else np.asarray(sigma, dtype=np.float64)
    if s.ndim == 0:
        s = np.full(n, float(s))
    if s.shape != (n,) or not np.isfinite(s).all() or (s <= 0).any():
        raise ValueError(f"{name} must be a positive, finite scalar or ({n},) vector, got {sigma!r}")
    return (np.float32(1) / s.astype(np.float32) ** 2).astype(np.float32)


def _check_report(states: np.ndarray, quat_adr: Sequence[int], what: str = "states") -> None:
    """A free joint's quaternion is reported whole or not at all: a part of it names no orientation, and the kernel could not align it."""
    states = np.atleast_2d(states)
    for a in quat_adr:
        n = np.isnan(states[..., a : a + 4]).sum(axis=-1)
        bad = np.argwhere((n > 0) & (n < 4))
        if bad.size:
            raise ValueError(f"{what}: the quaternion at offset {a} is reported in part in row {int(bad[0][-1])} ({int(n[tuple(bad[0])])} of its four coordinates are NaN); "
                             f"report a free joint's orientation whole or not at all")


def _residuals_reports(pred, obs, weight, quat_adr, pred_sens, obs_sens, weight_sens, plant_stride: int, window_stride: int, M: int, nq: int) -> np.ndarray:
    """(M, W) fp32 on the host: ONE `jh_plant_residuals_reports` call on device tensors."""
    from judo_amd.device import current_stream_ptr

    W, H, nx = obs.shape
    ns = 0 if obs_sens is None else int(obs_sens.shape[-1])
    err = torch.empty((M, W), dtype=torch.float32, device=obs.device)
    quats = (C.c_int * len(quat_adr))(*quat_adr) if quat_adr else None
    st = _lib.lib().jh_plant_residuals_reports(_lib.ptr(pred), _lib.ptr(obs), _lib.ptr(weight), quats, len(quat_adr), _lib.ptr(pred_sens) if ns else None,
                                               _lib.ptr(obs_sens) if ns else None, _lib.ptr(weight_sens) if ns else None, ns, plant_stride, window_stride, M, W, H, nx, nq,
                                               _lib.ptr(err), W, current_stream_ptr())
    _lib.check(st, "jh_plant_residuals_reports")
    return err.cpu().numpy()


class ReportEstimator(PlantEstimator):
    """`PlantEstimator` for a robot's reports: a posterior over the M plants of a `GpuModelSet` (cartpole, cylinder_push, the leap family, fr3_pick) from windows whose
    observations may hold NaN -- not reported, no evidence -- and whose sensor readings can be evidence beside the states.

        est = ReportEstimator(model_set, horizon=8, windows=16, sensor_sigma=0.01)   # or ReportEstimator.for_controller(ctrl, ...)
        est.observe(x0, controls, states, sensors)     # one window; states (horizon, nx) and sensors (horizon, ns) hold NaN where nothing was reported
        est.start(x); est.step(u, report); est.step(u)  # reports slower than the model: a model step at a time, the state after it or None
        posterior = est.update()                       # one plants launch, one jh_plant_residuals_reports call; est.errors, est.reported, est.map

    `x0` and the controls are always known.  A free joint's quaternion is reported whole or not at all.  `sensor_sigma` None: sensors are no evidence and the prediction
    launch asks for none; otherwise a positive scalar or (ns,) vector, and `sensors` omitted records a window whose sensor rows are all NaN.  `reported` counts the
    reported entries of every filled window; a window with none is no evidence: its error is exactly 0 for every plant.  Everything else -- the ring buffer, `observe_step`
    for full states, `state_sigma`, the prior, `temperature`, `discount`, `apply`, `apply_risk`, `for_controller` -- is `PlantEstimator`'s."""

    def __init__(self, model_set, horizon: int = 8, windows: int = 16, state_sigma=None, sensor_sigma=None, prior=None, temperature: float = 1.0, discount: float = 1.0,
                 _controller=None) -> None:
        super().__init__(model_set, horizon=horizon, windows=windows, state_sigma=state_sigma, prior=prior, temperature=temperature, discount=discount, _controller=_controller)
        self.ns = int(model_set.models[0].ns)
        if sensor_sigma is None:
            self.weight_sens = None
        else:
            if self.ns < 1:
                raise ValueError(f"sensor_sigma = {sensor_sigma!r} for a model without sensors (ns = 0): its sensors cannot be evidence")
            self.weight_sens = _check_sigma(sensor_sigma, self.ns, "sensor_sigma")
        self._obs_sens = self._weight_sens_d = None
        self._reported = np.zeros(self.windows, dtype=np.int64)  # per slot of the ring buffer

    # ---- recording -----------------------------------------------------------------------------------------------------------------------------------------------
    def reset(self, prior=None) -> None:
        super().reset(prior)
        self._window = None  # the window `start` / `step` are filling: dict(x0, controls, states, sensors)
        self.needs_start = True

    def _check_sensors(self, sensors, shape: tuple, what: str):
        if sensors is None:
            return None if self.weight_sens is None else np.full(shape, np.nan, dtype=np.float32)
        if self.weight_sens is None:
            raise ValueError("sensors are given, but the estimator was made with sensor_sigma = None: sensors are no evidence")
        sensors = _host(sensors)
        if sensors.shape != shape:
            raise ValueError(f"sensors must be {what} = {shape}, got {sensors.shape}")
        return sensors

    def observe(self, x0, controls, states, sensors=None) -> None:
        """Record one window: from state `x0` (nx,), `controls` (horizon, nu) were applied; `states` (horizon, nx), states[t] after controls[t], and `sensors` (horizon, ns)
        are what was reported, NaN elsewhere."""
        x0, controls, states = _host(x0), _host(controls), _host(states)
        H, nx, nu = self.horizon, self.nx, self.nu
        if x0.shape != (nx,):
            raise ValueError(f"x0 must be (nx,) = ({nx},), got {x0.shape}")
        if controls.shape != (H, nu):
            raise ValueError(f"controls must be (horizon, nu) = ({H}, {nu}), got {controls.shape}")
        if states.shape != (H, nx):
            raise ValueError(f"states must be (horizon, nx) = ({H}, {nx}), got {states.shape}")
        if np.isnan(x0).any():
            raise ValueError("x0 holds NaN: a window starts at a fully known state (only the states and sensors after it may be unreported)")
        if np.isnan(controls).any():
            raise ValueError("controls hold NaN: the controls the robot applied are known (only the states and sensors after them may be unreported)")
        _check_report(states, self.quat_adr)
        sensors = self._check_sensors(sensors, (H, self.ns), "(horizon, ns)")
        slot = self._pushed % self.windows
        super().observe(x0, controls, states)
        count = int((~np.isnan(states)).sum())
        if sensors is not None:
            if self._obs_sens is None:
                self._obs_sens = torch.zeros((self.windows, H, self.ns), dtype=torch.float32, device=self.device)
            self._obs_sens[slot].copy_(torch.from_numpy(np.ascontiguousarray(sensors, dtype=np.float32)))
            count += int((~np.isnan(sensors)).sum())
        self._reported[slot] = count

    def start(self, x) -> None:
        """Begin a pending window at the fully known state `x` (nx,); a pending one is dropped."""
        x = np.array(_host(x), dtype=np.float64)
        if x.shape != (self.nx,):
            raise ValueError(f"x must be (nx,) = ({self.nx},), got {x.shape}")
        if np.isnan(x).any():
            raise ValueError("x holds NaN: a window starts at a fully known state")
        self._window = dict(x0=x, controls=[], states=[], sensors=[])
        self.needs_start = False

    def step(self, u, report=None, sensors=None) -> None:
        """One model step under `u` (nu,): `report` (nx,) is the state after it, NaN where not reported, or None for no report; `sensors` (ns,) likewise.  After `horizon`
        steps the window is pushed; if its last report is a full state that state starts the next window, otherwise `needs_start` is True and `step` raises until
        `start` is called."""
        if self.needs_start or self._window is None:
            raise ValueError("no window is pending: the last window did not end in a full state (or none was begun); call start(x) with a fully known state")
        u = np.array(_host(u), dtype=np.float64)
        if u.shape != (self.nu,):
            raise ValueError(f"u must be (nu,) = ({self.nu},), got {u.shape}")
        if np.isnan(u).any():
            raise ValueError("u holds NaN: the controls the robot applied are known")
        report = np.full(self.nx, np.nan) if report is None else np.array(_host(report), dtype=np.float64)
        if report.shape != (self.nx,):
            raise ValueError(f"report must be (nx,) = ({self.nx},) or None, got {report.shape}")
        _check_report(report, self.quat_adr, "report")
        sensors = self._check_sensors(sensors, (self.ns,), "(ns,)")
        w = self._window
        w["controls"].append(u)
        w["states"].append(report)
        w["sensors"].append(sensors)
        if len(w["states"]) == self.horizon:
            self._window = None
            self.observe(w["x0"], np.stack(w["controls"]), np.stack(w["states"]), None if self.weight_sens is None else np.stack(w["sensors"]))
            if np.isnan(report).any():
                self.needs_start = True
            else:
                self.start(report)

    @property
    def window_steps(self) -> int:
        """Steps of the window `step` is filling."""
        return 0 if self._window is None else len(self._window["states"])

    @property
    def reported(self) -> np.ndarray:
        """(W,) int64: the reported entries, states and sensors, of every filled window, oldest first -- the columns of `errors`."""
        return self._reported[self._slots()].copy()

    def recorded_sensors(self) -> np.ndarray | None:
        """(W, horizon, ns) fp32, the sensor reports of the filled windows, oldest first (None where sensors are no evidence)."""
        if self.weight_sens is None:
            return None
        if not len(self) or self._obs_sens is None:
            return np.zeros((0, self.horizon, self.ns), np.float32)
        return self._obs_sens[torch.as_tensor(self._slots(), dtype=torch.long, device=self.device)].cpu().numpy()

    # ---- the update ----------------------------------------------------------------------------------------------------------------------------------------------
    def _predict_reports(self):
        """(pred, pred_sens, obs, obs_sens) on the device, the filled windows oldest first: ONE materialise launch on the set, M blocks of W rows, with sensors only when
        they are evidence."""
        from judo_amd.rollout_backend import GpuRolloutBackend

        ms, W = self.model_set, len(self)
        if len(ms.models) != self.num_plants:
            raise ValueError(f"model_set now has {len(ms.models)} plants, the estimator was made for M = {self.num_plants}")
        x0, controls, obs = self._recorded_device()
        want = self.weight_sens is not None
        pred, pred_sens = GpuRolloutBackend(ms.models[0], W).rollout_plants_device(ms, range(self.num_plants), x0.repeat(self.num_plants, 1), controls, shared_controls=True,
                                                                                   want_sensors=want)
        obs_sens = self._obs_sens[torch.as_tensor(self._slots(), dtype=torch.long, device=self.device)].contiguous() if want else None
        return pred, pred_sens, obs.contiguous(), obs_sens

    def _score(self) -> np.ndarray:
        pred, pred_sens, obs, obs_sens = self._predict_reports()
        if self._weight_d is None:
            self._weight_d = torch.from_numpy(self.weight).to(self.device)
        if self.weight_sens is not None and self._weight_sens_d is None:
            self._weight_sens_d = torch.from_numpy(self.weight_sens).to(self.device)
        return _residuals_reports(pred, obs, self._weight_d, self.quat_adr, pred_sens, obs_sens, self._weight_sens_d, len(self), 1, self.num_plants, self.nq)  # plant-major


class SpotReportEstimator(PlantBelief):
    """A posterior over the M plants of a `SpotPlantSet` from a robot's reports at the control rate.

        est = SpotReportEstimator(plants, horizon=4, windows=16)       # or SpotReportEstimator.for_controller(ctrl), which reads ctrl.plants on every update()
        est.observe(x0, commands, last_policy_output, states, sensors)  # one window of `horizon` control steps
        posterior = est.update(); est.apply_risk(ensemble_ctrl)         # or est.apply(randomised_ctrl)

    A window is T = `horizon` control steps and carries the policy state the Spot rollout needs: `x0` (nx,), `commands` (T, 25) as `task_to_sim_ctrl` gives them,
    `last_policy_output` (12,) -- the policy's output before the window's first step --, `states` (T, nx) where row i is the state after command row i's policy step and
    `physics_substeps` engine steps (`jh_policy_rollout`), and optionally `sensors` (T, nsensordata).  NaN in `states` and `sensors` means not reported; the
    quaternions of the description's free joints (the base, and the object where there is one) are reported whole or not at all and compared up to sign.

    `update()` is one `jh_policy_rollout_plants` chain with a problem per window -- G = M blocks of one rollout, block g on plant g, the window's policy output repeated
    M times, the warm start reset at every control step, no deadline -- in chunks of floor(JH_MAX_FLEET_PLANT_BLOCKS / M) windows where W * M exceeds that limit, then
    one `jh_plant_residuals_reports` call with window-major strides and the posterior in fp64 on the host.  The estimator owns what the chain mutates: a
    `PolicyRolloutBackend` of its own around the shared engine and policy handles, and a clone of the policy outputs; a controller's carried state is never touched."""

    def __init__(self, plants, horizon: int = 4, windows: int = 16, physics_substeps: int = 2, policy=None, state_sigma=None, sensor_sigma=None, prior=None,
                 temperature: float = 1.0, discount: float = 1.0, _controller=None) -> None:
        if not hasattr(plants, "descriptions") or not hasattr(plants, "nsensordata") or len(plants.descriptions) < 1:
            raise ValueError(f"plants must be a SpotPlantSet, got {type(plants).__name__}")
        self._ctrl, self._set, self._policy = _controller, plants, policy
        self.num_plants, self.nq, self.nv, self.ns = len(plants.descriptions), int(plants.nq), int(plants.nv), int(plants.nsensordata)
        self.nx = self.nq + self.nv
        if self.num_plants > _lib.MAX_ENSEMBLE:
            raise ValueError(f"plants: M = {self.num_plants} exceeds the {_lib.MAX_ENSEMBLE} plants jh_plant_residuals_reports scores (include/judo_amd.h JH_MAX_ENSEMBLE)")
        self._init_belief(horizon, windows, prior, temperature, discount)
        if int(physics_substeps) != physics_substeps or int(physics_substeps) < 1:
            raise ValueError(f"physics_substeps = {physics_substeps} must be at least 1")
        self.physics_substeps = int(physics_substeps)
        self.weight = _check_sigma(state_sigma, self.nx, "state_sigma")
        if sensor_sigma is None:
            self.weight_sens = None
        else:
            if self.ns < 1:
                raise ValueError(f"sensor_sigma = {sensor_sigma!r} for a model without sensors (nsensordata = 0): its sensors cannot be evidence")
            self.weight_sens = _check_sigma(sensor_sigma, self.ns, "sensor_sigma")
        desc = plants.descriptions[0]
        lay = layout(desc)
        free = [lay.jnt_qposadr[j] + 3 for j, jn in enumerate(desc["joints"]) if jn["type"] == "free"]
        if len(free) > MAX_ID_QUATS:
            raise ValueError(f"plants: {len(free)} free joints exceed the {MAX_ID_QUATS} quaternions jh_plant_residuals_reports aligns (include/judo_amd.h JH_MAX_ID_QUATS)")
        self.quat_adr = check_quat_adr(free, self.nq)
        self.device = plants.device
        self._x0 = self._commands = self._policy_out = self._obs = self._obs_sens = self._weight_d = self._weight_sens_d = None  # the ring buffer, made at the first window
        self._reported = np.zeros(self.windows, dtype=np.int64)
        self._backend = None
        self.reset()

    @classmethod
    def for_controller(cls, ctrl, **settings) -> "SpotReportEstimator":
        """The estimator of a `SpotEnsembleController` or a `SpotRandomizedController`.  `ctrl.plants` is read on every `update()`, so a plant replaced with `set_member`
        is scored as it now is; the policy and the substeps are those of `ctrl.rollout_backend`."""
        if not getattr(ctrl, "_spot_plants", False) or not hasattr(ctrl, "plants"):
            raise ValueError(f"ctrl is a {type(ctrl).__name__}, which plans on no SpotPlantSet: a SpotReportEstimator identifies the plants of a SpotEnsembleController or a "
                             f"SpotRandomizedController (judo_amd.spot_plants); identify.PlantEstimator and reports.ReportEstimator serve the controllers over a GpuModelSet")
        own = ctrl.rollout_backend
        return cls(ctrl.plants, physics_substeps=own.physics_substeps, policy=own.policy, _controller=ctrl, **settings)

    @property
    def plants(self):
        """The set the next `update()` scores: the controller's own as it now is, or the one given at construction."""
        return self._ctrl.plants if self._ctrl is not None else self._set

    # ---- recording -----------------------------------------------------------------------------------------------------------------------------------------------
    def observe(self, x0, commands, last_policy_output, states, sensors=None) -> None:
        """Record one window of T = `horizon` control steps (the class comment names its parts)."""
        x0, commands, pout, states = _host(x0), _host(commands), _host(last_policy_output), _host(states)
        T, nx = self.horizon, self.nx
        if x0.shape != (nx,):
            raise ValueError(f"x0 must be (nx,) = ({nx},), got {x0.shape}")
        if commands.shape != (T, POLICY_COMMAND_DIM):
            raise ValueError(f"commands must be (horizon, 25) = ({T}, {POLICY_COMMAND_DIM}), got {commands.shape}")
        if pout.shape != (POLICY_OUTPUT_DIM,):
            raise ValueError(f"last_policy_output must be ({POLICY_OUTPUT_DIM},), got {pout.shape}")
        if states.shape != (T, nx):
            raise ValueError(f"states must be (horizon, nx) = ({T}, {nx}), got {states.shape}")
        for a, name in ((x0, "x0"), (commands, "commands"), (pout, "last_policy_output")):
            if np.isnan(a).any():
                raise ValueError(f"{name} holds NaN: what a window starts from and the commands the robot was given are known (only the states and sensors may be unreported)")
        _check_report(states, self.quat_adr)
        if sensors is None:
            sensors = None if self.weight_sens is None else np.full((T, self.ns), np.nan, dtype=np.float32)
        elif self.weight_sens is None:
            raise ValueError("sensors are given, but the estimator was made with sensor_sigma = None: sensors are no evidence")
        else:
            sensors = _host(sensors)
            if sensors.shape != (T, self.ns):
                raise ValueError(f"sensors must be (horizon, nsensordata) = ({T}, {self.ns}), got {sensors.shape}")
        if self._x0 is None:
            def ring(*shape):
                return torch.zeros((self.windows,) + shape, dtype=torch.float32, device=self.device)

            self._x0, self._commands, self._policy_out, self._obs = ring(nx), ring(T, POLICY_COMMAND_DIM), ring(POLICY_OUTPUT_DIM), ring(T, nx)
            self._obs_sens = ring(T, self.ns) if self.weight_sens is not None else None
        slot = self._pushed % self.windows
        bufs = [(self._x0, x0), (self._commands, commands), (self._policy_out, pout), (self._obs, states)] + ([(self._obs_sens, sensors)] if sensors is not None else [])
        for buf, a in bufs:
            buf[slot].copy_(torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)))
        self._reported[slot] = int((~np.isnan(states)).sum()) + (int((~np.isnan(sensors)).sum()) if sensors is not None else 0)
        self._pushed += 1
        self._posterior = None

    def _recorded_device(self) -> list:
        """[x0, commands, last_policy_output, states, sensors or None] of the filled windows on the device, oldest first."""
        idx = torch.as_tensor(self._slots(), dtype=torch.long, device=self.device)
        return [None if t is None else t[idx].contiguous() for t in (self._x0, self._commands, self._policy_out, self._obs, self._obs_sens)]

    def recorded(self) -> tuple:
        """(x0 (W, nx), commands (W, T, 25), last_policy_output (W, 12), states (W, T, nx), sensors (W, T, ns) or None) of the W filled windows as fp32 host arrays,
        oldest first: the columns of `errors`."""
        T = self.horizon
        if not len(self):
            empty = [np.zeros((0,) + s, np.float32) for s in ((self.nx,), (T, POLICY_COMMAND_DIM), (POLICY_OUTPUT_DIM,), (T, self.nx), (T, self.ns))]
            return tuple(empty[:4]) + (empty[4] if self.weight_sens is not None else None,)
        return tuple(None if t is None else t.cpu().numpy() for t in self._recorded_device())

    @property
    def reported(self) -> np.ndarray:
        """(W,) int64: the reported entries, states and sensors, of every filled window, oldest first."""
        return self._reported[self._slots()].copy()

    # ---- the update ----------------------------------------------------------------------------------------------------------------------------------------------
    def chunks(self, W: int | None = None) -> list[tuple[int, int]]:
        """The contiguous ranges [a, b) of windows that one launch chain each rolls out: floor(JH_MAX_FLEET_PLANT_BLOCKS / M) windows to a chain."""
        W, per = len(self) if W is None else int(W), MAX_FLEET_PLANT_BLOCKS // self.num_plants
        return [(a, min(a + per, W)) for a in range(0, W, per)]

    def _rollout_backend(self, rows: int):
        """The estimator's own backend of `rows` threads around the controller's (or its own) engine and policy handles: its warm start is the estimator's."""
        from judo_amd.policy import PolicyRolloutBackend, SpotLocomotionPolicy

        plants = self.plants
        if self._ctrl is not None:
            share = self._ctrl.rollout_backend
        else:
            if self._policy is None:
                self._policy = SpotLocomotionPolicy(device=self.device)
            share = SimpleNamespace(device=self.device, engine=plants.engines[0], policy=self._policy)
        pb = self._backend
        if pb is None or pb.policy is not share.policy or pb.engine is not share.engine:
            pb = self._backend = PolicyRolloutBackend(rows, physics_substeps=self.physics_substeps, device=self.device, carry_warmstart=False, share=share)
        if pb.num_threads != rows:
            pb.update(rows)
        return pb

    def _predict_reports(self):
        """(pred, pred_sens, obs, obs_sens) on the device, the filled windows oldest first; pred (W * M, T, nx) window-major, row w * M + m."""
        plants, M = self.plants, self.num_plants
        if len(plants.descriptions) != M:
            raise ValueError(f"plants now has {len(plants.descriptions)} members, the estimator was made for M = {M}")
        x0, commands, pout, obs, obs_sens = self._recorded_device()
        states, sensors = [], []
        for a, b in self.chunks():
            B = b - a
            pb = self._rollout_backend(B * M)
            s, y = pb.rollout_plants(plants, x0[a:b].contiguous(), self.nx, B, M, list(range(M)) * B, commands[a:b].repeat_interleave(M, dim=0).contiguous(),
                                     pout[a:b].repeat_interleave(M, dim=0).clone().contiguous(), cutoff_time=None)
            states.append(s)
            sensors.append(y)
        want = self.weight_sens is not None
        pred = states[0] if len(states) == 1 else torch.cat(states)
        pred_sens = (sensors[0] if len(sensors) == 1 else torch.cat(sensors)) if want else None
        return pred, pred_sens, obs, obs_sens if want else None

    def _score(self) -> np.ndarray:
        pred, pred_sens, obs, obs_sens = self._predict_reports()
        if self._weight_d is None:
            self._weight_d = torch.from_numpy(self.weight).to(self.device)
        if self.weight_sens is not None and self._weight_sens_d is None:
            self._weight_sens_d = torch.from_numpy(self.weight_sens).to(self.device)
        return _residuals_reports(pred, obs, self._weight_d, self.quat_adr, pred_sens, obs_sens, self._weight_sens_d, 1, self.num_plants, self.num_plants, self.nq)  # window-major


__all__ = ["MAX_FLEET_PLANT_BLOCKS", "ReportEstimator", "SpotReportEstimator", "plant_residuals_reports_host"]
