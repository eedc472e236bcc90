"""Identify the plant: a posterior over the M members of a `GpuModelSet` from observed steps (`jh_plant_residuals`, include/judo_amd.h).

The controllers of judo_amd/ensemble.py, randomized.py and materialized.py (and their fr3 forms) plan against a set of plausible plants whose weights are the user's guess.
The robot produces the evidence that settles the guess on every control step: it applied `u` in state `x` and arrived at `x'`.  A `PlantEstimator` records such steps in
windows of `horizon` model steps, rolls every recorded window out on all M plants in ONE materialise launch on the set (`GpuRolloutBackend.rollout_plants_device`: M
blocks of W rows, the windows' controls shared), scores the predictions against the observations in ONE `jh_plant_residuals` call, and turns the (M, W) errors into a
posterior on the host in fp64.  `apply` hands the posterior to a randomised controller as its next assignment (`Assignment.set_weights`: no device cost).

`plant_residuals_host` restates the kernel's arithmetic in numpy fp32, operation for operation; the device result equals it bit for bit
(tests/test_gpu_plant_residuals.py).  `posterior_from_errors` is the posterior arithmetic alone.  The reference has no counterpart."""

from __future__ import annotations

import ctypes as C
from typing import Sequence

import numpy as np
import torch

from judo_amd import _lib
from judo_amd.models import layout
from judo_amd.plants import Assignment, WorstCase

MAX_ID_HORIZON = _lib.MAX_ID_HORIZON
MAX_ID_QUATS = _lib.MAX_ID_QUATS


def check_quat_adr(quat_adr: Sequence[int], nq: int) -> list[int]:
    """`quat_adr` as a list of at most MAX_ID_QUATS offsets whose four coordinates lie in [0, nq) and do not overlap (the rule of `jh_plant_residuals`); raises ValueError."""
    q = [int(a) for a in quat_adr]
    if len(q) > MAX_ID_QUATS:
        raise ValueError(f"nquat = {len(q)} outside [0, {MAX_ID_QUATS}] (include/judo_amd.h JH_MAX_ID_QUATS)")
    for i, a in enumerate(q):
        if not 0 <= a <= nq - 4:
            raise ValueError(f"quat_adr[{i}] = {a}: its four coordinates do not lie in [0, nq = {nq})")
        for j in range(i):
            if abs(a - q[j]) < 4:
                raise ValueError(f"quat_adr[{i}] = {a} overlaps quat_adr[{j}] = {q[j]}")
    return q


def plant_residuals_host(pred, obs, weight, quat_adr: Sequence[int] = (), nq: int | None = None) -> np.ndarray:
    """The weighted squared prediction error of every plant on every window, (M, W) fp32, from `pred` (M * W, H, nx) -- block m = rows [m * W, (m + 1) * W) --, `obs`
    (W, H, nx), `weight` (nx) and the quaternion offsets `quat_adr` (inside [0, `nq`), None: nx).  What `jh_plant_residuals` computes, bit for bit, every product and sum
    rounded to fp32 on its own: per step and quaternion dot = ((p0 * o0 + p1 * o1) + p2 * o2) + p3 * o3, and where dot < 0 the prediction is compared against -o; per
    coordinate e = p - o', t = (weight * e) * e; per step the t are added in ascending d; per window the H step sums are placed in 64 slots, the rest +0.0, and halved six
    times (v[i] = v[i] + v[i + k], k = 32, 16, 8, 4, 2, 1).  NaN in gives NaN out."""
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
    p = p.reshape(M, W, H, nx)
    oo = np.broadcast_to(o, p.shape).copy()
    with np.errstate(over="ignore", invalid="ignore"):
        for a in quats:
            dot = p[..., a] * o[..., a]
            for i in (1, 2, 3):
                dot = dot + p[..., a + i] * o[..., a + i]
            oo[..., a : a + 4] = np.where((dot < 0)[..., None], -o[..., a : a + 4], o[..., a : a + 4])
        e = p - oo
        t = (wt * e) * e
        s = t[..., 0].copy()
        for d in range(1, nx):
            s = s + t[..., d]
        v = np.zeros((M, W, 64), dtype=np.float32)
        v[..., :H] = s
        for k in (32, 16, 8, 4, 2, 1):
            v[..., :k] = v[..., :k] + v[..., k : 2 * k]
    assert v.dtype == np.float32
    return v[..., 0].copy()


def check_prior(prior, M: int) -> np.ndarray:
    """`prior` as (M,) fp64 that adds up to 1 (None: uniform); raises ValueError naming it: the wrong length, a negative or non-finite entry, a zero sum."""
    if prior is None:
        return np.full(M, 1.0 / M)
    p = np.asarray(prior, dtype=np.float64).reshape(-1)
    if p.size != M:
        raise ValueError(f"prior has {p.size} entries for M = {M} plants")
    if not np.isfinite(p).all() or (p < 0).any():
        raise ValueError(f"prior must be non-negative, finite numbers, got {list(p)}")
    if p.sum() <= 0:
        raise ValueError(f"prior has zero sum: {list(p)}")
    return p / p.sum()


def posterior_from_errors(errors, prior, temperature: float = 1.0, discount: float = 1.0) -> tuple[np.ndarray, np.ndarray, bool]:
    """(posterior, log_likelihood, degenerate) in fp64 from `errors` (M, W), the windows in the order they were recorded: the newest is the last column and has age 0.
    L[m] = 0.5 * sum_w discount**age_w * errors[m, w]; log_likelihood = -L; logp = log(prior) - L / temperature; posterior = softmax(logp).  A non-finite error counts
    as +inf: that plant has likelihood zero.  If no member has a finite logp, the posterior is the prior and `degenerate` is True."""
    e = np.asarray(errors, dtype=np.float64)
    if e.ndim != 2:
        raise ValueError(f"errors must be (M, W), got {e.shape}")
    M, W = e.shape
    prior = check_prior(prior, M)
    if not temperature > 0:
        raise ValueError(f"temperature = {temperature} must be positive")
    if not 0 < discount <= 1:
        raise ValueError(f"discount = {discount} outside (0, 1]")
    e = np.where(np.isfinite(e), e, np.inf)
    age = np.arange(W - 1, -1, -1, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        terms = np.where(np.isinf(e), np.inf, float(discount) ** age * e)  # (an infinite error stays infinite however old: a discount that underflowed gives 0 * inf)
    L = 0.5 * terms.sum(axis=1) if W else np.zeros(M)
    with np.errstate(divide="ignore"):
        logp = np.log(prior) - L / float(temperature)
    live = np.isfinite(logp)
    if not live.any():
        return prior.copy(), -L, True
    z = np.where(live, np.exp(np.where(live, logp - logp[live].max(), 0.0)), 0.0)
    return z / z.sum(), -L, False


def _host(a) -> np.ndarray:
    return a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)


def _refuse_spot(what) -> None:
    if type(what).__name__ == "SpotPlantSet":
        raise ValueError("model_set is a SpotPlantSet: the Spot policy rollout carries policy state (the policy outputs and the warm start) that a recorded window would have "
                         "to include, which a PlantEstimator does not record; it identifies the plants of a GpuModelSet")


class PlantBelief:
    """What every estimator of the plant shares (`PlantEstimator` here, `ReportEstimator` and `SpotReportEstimator` of judo_amd/reports.py): the count of windows in a ring
    buffer of `windows` slots, the posterior arithmetic on the (M, filled windows) errors a subclass's `_score` returns, and the hand-over to a controller.  A subclass
    sets `num_plants` and calls `_init_belief`, owns the ring buffer's tensors, and advances `_pushed` when it records a window."""

    def _init_belief(self, horizon, windows, prior, temperature: float, discount: float) -> None:
        if int(horizon) != horizon or not 1 <= int(horizon) <= MAX_ID_HORIZON:
            raise ValueError(f"horizon = {horizon} outside [1, {MAX_ID_HORIZON}] (include/judo_amd.h JH_MAX_ID_HORIZON)")
        if int(windows) != windows or int(windows) < 1:
            raise ValueError(f"windows = {windows} must be at least 1")
        self.horizon, self.windows = int(horizon), int(windows)
        if not temperature > 0:
            raise ValueError(f"temperature = {temperature} must be positive")
        if not 0 < discount <= 1:
            raise ValueError(f"discount = {discount} outside (0, 1]")
        self.temperature, self.discount = float(temperature), float(discount)
        self._prior0 = self.prior = check_prior(prior, self.num_plants)

    def reset(self, prior=None) -> None:
        """Empty the ring buffer and the pending window; `prior` replaces the prior (None: the one of construction)."""
        self.prior = self._prior0 if prior is None else check_prior(prior, self.num_plants)
        self._pushed = 0  # windows pushed since the reset: window i lives in slot i % windows
        self._pending: list[tuple[np.ndarray, np.ndarray, np.ndarray]] = []
        self._posterior = None
        self.errors = np.zeros((self.num_plants, 0), dtype=np.float32)
        self.log_likelihood = np.zeros(self.num_plants)
        self.degenerate = False

    def __len__(self) -> int:
        return min(self._pushed, self.windows)

    def _slots(self) -> list[int]:
        """The filled slots of the ring buffer, oldest window first."""
        return [i % self.windows for i in range(max(0, self._pushed - self.windows), self._pushed)]

    def update(self) -> np.ndarray:
        """The posterior over the M plants, (M,) fp64, from the filled windows (the prior with none).  Leaves `errors` (M, filled windows; oldest first), `log_likelihood`
        (M,: -0.5 * the discounted sum of a plant's errors, before the temperature), `map` and `degenerate` behind."""
        self.errors = self._score() if len(self) else np.zeros((self.num_plants, 0), dtype=np.float32)
        self._posterior, self.log_likelihood, self.degenerate = posterior_from_errors(self.errors, self.prior, self.temperature, self.discount)
        return self._posterior.copy()

    @property
    def posterior(self) -> np.ndarray:
        """The posterior of the windows recorded so far (`update()` if a window arrived since the last one)."""
        if self._posterior is None:
            self.update()
        return self._posterior.copy()

    @property
    def map(self) -> int:
        """The plant of largest posterior, ties to the lower index."""
        return int(np.argmax(self.posterior))

    # ---- the hand-over -------------------------------------------------------------------------------------------------------------------------------------------
    def apply(self, ctrl, floor: float = 0.25) -> np.ndarray:
        """A randomised controller's next assignment from the posterior: `ctrl.set_weights((1 - floor) * posterior + floor / M)`, returned.  With `floor` > 0 every plant
        keeps a remainder in the apportionment (`plants.blocks_from_weights`), so evidence against the current belief can still arrive.  `ctrl` is a controller with an
        `Assignment`: `RandomizedController`, `MaterializedRandomizedController` and their fr3 forms.  An ensemble controller is refused here: it has no assignment; `apply_risk`
        hands it the posterior as the weights of its plant-weighted risk measure."""
        if not 0 <= floor <= 1:
            raise ValueError(f"floor = {floor} outside [0, 1]")
        if isinstance(ctrl, WorstCase):
            raise ValueError(f"ctrl is a {type(ctrl).__name__}, an ensemble controller: its risk measure has no plant weights (a plant-weighted risk measure is out of "
                             f"scope).  Follow the belief with ctrl.set_member on the MAP plant's neighbours, or prune the set")
        if not isinstance(ctrl, Assignment):
            raise ValueError(f"ctrl is a {type(ctrl).__name__}, which has no assignment of rollout blocks to plants: apply needs a RandomizedController, a "
                             f"MaterializedRandomizedController or one of their fr3 forms")
        w = (1.0 - float(floor)) * self.posterior + float(floor) / self.num_plants
        ctrl.set_weights(w)
        return w

    def apply_risk(self, ctrl, floor: float = 0.0, tail: float | None = None) -> np.ndarray:
        """An ensemble controller's plant-weighted risk measure from the posterior: `ctrl.set_weights((1 - floor) * posterior + floor / M, tail)`, the weights returned.
        From the next plan step on a candidate's cost is the tail mean of its member costs under these weights (`plants.WorstCase.set_weights`), so a plant the
        observed steps have ruled out no longer drives the plan.  `floor` > 0 keeps every plant at a positive weight; `tail` None keeps the controller's tail mass.
        `ctrl` is a controller with a `WorstCase`: `EnsembleController`, `MaterializedEnsembleController`, their fr3 forms and `SpotEnsembleController`; a randomised
        controller follows the belief with `apply`."""
        if not 0 <= floor <= 1:
            raise ValueError(f"floor = {floor} outside [0, 1]")
        if not isinstance(ctrl, WorstCase):
            raise ValueError(f"ctrl is a {type(ctrl).__name__}, which has no risk measure over its plants: apply_risk needs an EnsembleController, a "
                             f"MaterializedEnsembleController, one of their fr3 forms or a SpotEnsembleController"
                             + ("; a randomised controller follows the belief with apply" if isinstance(ctrl, Assignment) else ""))
        w = (1.0 - float(floor)) * self.posterior + float(floor) / self.num_plants
        ctrl.set_weights(w, tail)
        return w


class PlantEstimator(PlantBelief):
    """A posterior over the M plants of a `GpuModelSet` (cartpole, cylinder_push, the leap family, fr3_pick) from recorded windows of `horizon` model steps.

        est = PlantEstimator(model_set, horizon=8, windows=16)   # or PlantEstimator.for_controller(ctrl), which reads ctrl.model_set on every update()
        est.observe(x0, controls, states)                        # one window, as jh_rollout_materialize defines it: states[t] is the state after controls[t]
        est.observe_step(x, u, x_next)                           # one model step at a time; consecutive steps are chained into windows
        posterior = est.update()                                 # (M,) fp64; est.errors (M, filled windows), est.log_likelihood (M,), est.map, est.degenerate
        est.apply(ctrl, floor=0.25)                              # a randomised controller's next assignment from the posterior

    The states are the PLANT's states at the MODEL's own timestep, one per physics step, in the layout `RolloutBackend.rollout` returns (qpos then qvel); the controls are
    what the simulation takes (`task_to_sim_ctrl` applied).  Resampling a robot's slower or irregular observations onto the model's timestep is the caller's job.

    `windows` recorded windows live in a ring buffer of device tensors; when it is full the oldest is replaced.  `update()` is one materialise launch on the set followed
    by one `jh_plant_residuals` call, then the posterior in fp64 on the host (`posterior_from_errors`); with no window filled it returns the prior.  `state_sigma`, a
    positive scalar or (nx,) vector, is the observation noise: the errors are weighted by 1 / sigma**2 (default 1).  The quaternions of the description's free joints are
    compared up to sign.  `temperature` > 0 flattens the likelihood, `discount` in (0, 1] weighs a window of age a (the newest has age 0) by discount**a."""

    def __init__(self, model_set, horizon: int = 8, windows: int = 16, state_sigma=None, prior=None, temperature: float = 1.0, discount: float = 1.0, _controller=None) -> None:
        _refuse_spot(model_set)
        if not hasattr(model_set, "models") or len(model_set.models) < 1:
            raise ValueError(f"model_set must be a GpuModelSet, got {type(model_set).__name__}")
        self._ctrl, self._set = _controller, model_set
        first = model_set.models[0]
        self.num_plants, self.nx, self.nu, self.nq = len(model_set.models), int(first.nx), int(first.nu), int(first.nq)
        self._init_belief(horizon, windows, prior, temperature, discount)
        sigma = np.ones(self.nx) if state_sigma is None else np.asarray(state_sigma, dtype=np.float64)
        if sigma.ndim == 0:
            sigma = np.full(self.nx, float(sigma))
        if sigma.shape != (self.nx,) or not np.isfinite(sigma).all() or (sigma <= 0).any():
            raise ValueError(f"state_sigma must be a positive, finite scalar or ({self.nx},) vector, got {state_sigma!r}")
        self.weight = (np.float32(1) / sigma.astype(np.float32) ** 2).astype(np.float32)
        lay, desc = layout(first.desc), first.desc
        free = [lay.jnt_qposadr[j] + 3 for j, jn in enumerate(desc["joints"]) if jn["type"] == "free"]
        if len(free) > MAX_ID_QUATS:
            raise ValueError(f"model_set: {len(free)} free joints exceed the {MAX_ID_QUATS} quaternions jh_plant_residuals aligns (include/judo_amd.h JH_MAX_ID_QUATS)")
        self.quat_adr = check_quat_adr(free, self.nq)
        self.device = first.device
        self._x0 = self._controls = self._obs = self._weight_d = None  # the ring buffer, made at the first window
        self.reset()

    @classmethod
    def for_controller(cls, ctrl, **settings) -> "PlantEstimator":
        """The estimator of a controller over a `GpuModelSet` -- ensemble, randomised, materialised, and their fr3 forms.  `ctrl.model_set` is read on every `update()`, so
        a plant replaced with `set_member` is scored as it now is."""
        _refuse_spot(getattr(ctrl, "plants", None))
        if not hasattr(ctrl, "model_set"):
            raise ValueError(f"ctrl is a {type(ctrl).__name__}, which plans on no GpuModelSet: a PlantEstimator identifies the plants of an ensemble, randomised or "
                             f"materialised controller (judo_amd.ensemble, randomized, materialized and their fr3 forms)")
        return cls(ctrl.model_set, _controller=ctrl, **settings)

    @property
    def model_set(self):
        """The set the next `update()` scores: the controller's own as it now is, or the one given at construction."""
        return self._ctrl.model_set if self._ctrl is not None else self._set

    # ---- recording -----------------------------------------------------------------------------------------------------------------------------------------------
    def _recorded_device(self) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """(x0, controls, states) of the filled windows on the device, oldest first."""
        W = len(self)
        if self._pushed <= self.windows:
            return self._x0[:W], self._controls[:W], self._obs[:W]
        idx = torch.as_tensor(self._slots(), dtype=torch.long, device=self.device)
        return self._x0[idx], self._controls[idx], self._obs[idx]

    def recorded(self) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
        """(x0 (W, nx), controls (W, horizon, nu), states (W, horizon, nx)) of the W filled windows as fp32 host arrays, oldest first: the columns of `errors`."""
        if not len(self):
            return (np.zeros((0, self.nx), np.float32), np.zeros((0, self.horizon, self.nu), np.float32), np.zeros((0, self.horizon, self.nx), np.float32))
        return tuple(t.cpu().numpy() for t in self._recorded_device())

    def observe(self, x0, controls, states) -> None:
        """Record one window: from state `x0` (nx,), `controls` (horizon, nu) were applied and `states` (horizon, nx) observed, states[t] after controls[t]."""
        x0, controls, states = _host(x0), _host(controls), _host(states)
        H, nx, nu = self.horizon, self.nx, self.nu
        if x0.shape != (nx,):
            raise ValueError(f"x0 must be (nx,) = ({nx},), got {x0.shape}")
        if controls.shape != (H, nu):
            raise ValueError(f"controls must be (horizon, nu) = ({H}, {nu}), got {controls.shape}")
        if states.shape != (H, nx):
            raise ValueError(f"states must be (horizon, nx) = ({H}, {nx}), got {states.shape}")
        if self._x0 is None:
            self._x0 = torch.zeros((self.windows, nx), dtype=torch.float32, device=self.device)
            self._controls = torch.zeros((self.windows, H, nu), dtype=torch.float32, device=self.device)
            self._obs = torch.zeros((self.windows, H, nx), dtype=torch.float32, device=self.device)
        slot = self._pushed % self.windows
        for buf, a in ((self._x0, x0), (self._controls, controls), (self._obs, states)):
            buf[slot].copy_(torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)))
        self._pushed += 1
        self._posterior = None

    def observe_step(self, x, u, x_next) -> None:
        """Record one model step: `u` (nu,) applied in state `x` (nx,) gave `x_next` (nx,).  Consecutive steps are chained into one pending window, which is pushed after
        `horizon` of them.  If `x` is not element for element the pending window's last `x_next`, the recording has a gap: the pending window is dropped and a new one
        starts at `x`.  One call per physics step of the model: resampling slower observations is the caller's job."""
        x, u, x_next = (np.array(_host(a), dtype=np.float64) for a in (x, u, x_next))
        if x.shape != (self.nx,) or x_next.shape != (self.nx,):
            raise ValueError(f"x and x_next must be (nx,) = ({self.nx},), got {x.shape} and {x_next.shape}")
        if u.shape != (self.nu,):
            raise ValueError(f"u must be (nu,) = ({self.nu},), got {u.shape}")
        if self._pending and not np.array_equal(self._pending[-1][2], x):
            self._pending = []
        self._pending.append((x, u, x_next))
        if len(self._pending) == self.horizon:
            steps, self._pending = self._pending, []
            self.observe(steps[0][0], np.stack([s[1] for s in steps]), np.stack([s[2] for s in steps]))

    @property
    def pending_steps(self) -> int:
        """Steps of the window `observe_step` is filling."""
        return len(self._pending)

    # ---- the update ----------------------------------------------------------------------------------------------------------------------------------------------
    def _predict(self) -> tuple[torch.Tensor, torch.Tensor]:
        """(pred, obs) on the device, the filled windows oldest first: pred (M * W, H, nx) from ONE materialise launch on the set, M blocks of W rows."""
        from judo_amd.rollout_backend import GpuRolloutBackend

        ms, W = self.model_set, len(self)
        _refuse_spot(ms)
        if len(ms.models) != self.num_plants:
            raise ValueError(f"model_set now has {len(ms.models)} plants, the estimator was made for M = {self.num_plants}")
        x0, controls, obs = self._recorded_device()
        pred, _ = GpuRolloutBackend(ms.models[0], W).rollout_plants_device(ms, range(self.num_plants), x0.repeat(self.num_plants, 1), controls, shared_controls=True,
                                                                           want_sensors=False)
        return pred, obs.contiguous()

    def _residuals(self, pred: torch.Tensor, obs: torch.Tensor) -> np.ndarray:
        """(M, W) fp32 on the host: ONE `jh_plant_residuals` call."""
        from judo_amd.device import current_stream_ptr

        M, (W, H, nx) = self.num_plants, obs.shape
        if self._weight_d is None:
            self._weight_d = torch.from_numpy(self.weight).to(self.device)
        err = torch.empty((M, W), dtype=torch.float32, device=self.device)
        quats = (C.c_int * len(self.quat_adr))(*self.quat_adr) if self.quat_adr else None
        st = _lib.lib().jh_plant_residuals(_lib.ptr(pred), _lib.ptr(obs), _lib.ptr(self._weight_d), quats, len(self.quat_adr), M, W, H, nx, self.nq, _lib.ptr(err), W,
                                           current_stream_ptr())
        _lib.check(st, "jh_plant_residuals")
        return err.cpu().numpy()

    def _score(self) -> np.ndarray:
        return self._residuals(*self._predict())


__all__ = ["MAX_ID_HORIZON", "MAX_ID_QUATS", "PlantBelief", "PlantEstimator", "check_prior", "check_quat_adr", "plant_residuals_host", "posterior_from_errors"]
