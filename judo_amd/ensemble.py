"""One controller planned against an ensemble of M plants (`jh_plan_step_ensemble`, include/judo_amd.h).

A `ControllerFleet` over M descriptions is M controllers with M nominals, each of which believes its own plant.  An `EnsembleController` is ONE controller with ONE
nominal spline: each of its N candidates is rolled out on all M members of a `GpuModelSet` -- one block, one noise slice, a model image per member -- and scored by a
risk measure over the M costs: the mean of the `worst` largest (`worst` = 1: the worst case, `worst` = M: the mean, in between a tail mean that stands in for CVaR).
MPPI / CEM / PS then run once on the aggregated costs, in the same launch that aggregates them.  The reference has no counterpart.

Member 0 is the nominal plant: the controller's `model`, on which the traces are re-rolled.  `aggregate_costs_host` restates the aggregation in numpy fp32, operation
for operation; the device result equals it bit for bit (tests/test_gpu_ensemble_costs.py)."""

from __future__ import annotations

from typing import Sequence

import numpy as np
import torch

from judo_amd import _lib
from judo_amd.config import ControllerConfig
from judo_amd.controller import Controller
from judo_amd.plants import MAX_ENSEMBLE, FusedPlantController, WorstCase, check_descriptions, make_for, materialized_hint
from judo_amd.tasks import Task


def aggregate_costs_host(member_costs, worst: int) -> np.ndarray:
    """The aggregated cost of every rollout, (N,) fp32, from `member_costs` (M, N): the `worst` largest of a rollout's M member costs are added in fp32 in descending
    order, starting from the largest, and the sum is divided by `worst` in fp32 (correctly rounded).  `worst` = 1 is the exact maximum, `worst` = M the mean.  +inf and
    the 3.0e38 sentinel behave as IEEE arithmetic makes them; NaN is outside the contract.  What `ensemble_cost` (judo_amd/csrc/jh_update_dev.h) computes, bit for bit."""
    c = np.asarray(member_costs, dtype=np.float32)
    if c.ndim != 2:
        raise ValueError(f"member_costs must be (M, N), got {c.shape}")
    M = c.shape[0]
    j = int(worst)
    if not 1 <= j <= M:
        raise ValueError(f"worst = {worst} outside [1, M = {M}]")
    top = -np.sort(-c, axis=0)[:j]  # the j largest per rollout, largest first (equal values are interchangeable)
    with np.errstate(over="ignore"):  # (3.0e38 + 3.0e38 = +inf, as on the device)
        acc = top[0].copy()
        for i in range(1, j):
            acc = (acc + top[i]).astype(np.float32)  # sequential fp32 adds
        return (acc / np.float32(j)).astype(np.float32)


def aggregate_costs_weighted_host(member_costs, weights, tail) -> np.ndarray:
    """The plant-weighted aggregated cost of every rollout, (N,) fp32, from `member_costs` (M, N): the tail mean (CVaR) of a rollout's M member costs under `weights`
    (M fp32 values, each finite and >= 0, at least one > 0) with the tail mass `tail`, fp32 in (0, 1], as include/judo_amd.h fixes it.  The distinct values are visited
    in strictly descending order; a value's weight ws is the sum of its members' weights in ascending m; take = min(ws, tail - got); a group with take > 0 adds
    take * value to the sum and take to the mass `got`; the result is the sum over `got`.  Every operation is rounded to fp32 on its own.  +inf and the 3.0e38 sentinel
    behave as IEEE arithmetic makes them; NaN costs are outside the contract.  What `ensemble_cost_weighted` (judo_amd/csrc/jh_update_dev.h) computes, bit for bit.
    Raises ValueError for what `jh_ensemble_costs_weighted` refuses."""
    c = np.asarray(member_costs, dtype=np.float32)
    if c.ndim != 2:
        raise ValueError(f"member_costs must be (M, N), got {c.shape}")
    M, N = c.shape
    if not 1 <= M <= MAX_ENSEMBLE:
        raise ValueError(f"M = {M} outside [1, JH_MAX_ENSEMBLE = {MAX_ENSEMBLE}]")
    if weights is None:
        raise ValueError("weights is None")
    with np.errstate(over="ignore"):
        p = np.asarray(weights, dtype=np.float32).reshape(-1)
    if p.size != M:
        raise ValueError(f"{p.size} weights for M = {M} plants")
    for m in range(M):
        if not (np.isfinite(p[m]) and p[m] >= 0):
            raise ValueError(f"weights[{m}] = {p[m]} is negative or not finite")
    if not (p > 0).any():
        raise ValueError(f"weights are all zero (M = {M}): at least one plant needs a positive weight")
    tail = np.float32(tail)
    if not (tail > 0 and tail <= 1):  # (false for NaN)
        raise ValueError(f"tail = {tail} outside (0, 1]")
    f32 = np.float32
    acc, got, hi = np.zeros(N, f32), np.zeros(N, f32), np.zeros(N, f32)
    started, live = np.zeros(N, bool), np.ones(N, bool)
    with np.errstate(over="ignore", invalid="ignore"):
        for step in range(M):  # one pass per distinct value, at most M
            cur, ws, have = np.zeros(N, f32), np.zeros(N, f32), np.zeros(N, bool)
            for m in range(M):
                x = c[m]
                is_open = live & (x < hi) if step else live.copy()  # not yet visited
                up = is_open & (~have | (x > cur))
                ws = np.where(up, p[m], np.where(is_open & (x == cur), (ws + p[m]).astype(f32), ws)).astype(f32)
                cur = np.where(up, x, cur)
                have |= is_open
            rem = (tail - got).astype(f32)
            take = np.where(ws < rem, ws, rem).astype(f32)
            add = have & (take > 0)
            t = (take * cur).astype(f32)
            acc = np.where(add, np.where(started, (acc + t).astype(f32), t), acc).astype(f32)
            got = np.where(add, (got + take).astype(f32), got).astype(f32)
            started |= add
            hi = np.where(have, cur, hi)
            live &= have & ~(got >= tail)
        return (acc / got).astype(f32)


def aggregate_costs_risk_batch_host(member_costs, worst, risk) -> np.ndarray:
    """The aggregated costs of B controllers, (B, N) fp32, from `member_costs` (B, M, N), `worst` (B,) and the controllers' risk records `risk` (B, 1 + M) as
    include/judo_amd.h fixes them for `jh_ensemble_costs_risk_batch`: a tail word of exactly 0 is the counted measure with `worst[b]` (`aggregate_costs_host`; the
    weights are not read), any other the tail mass of the plant-weighted one under the M weights behind it (`aggregate_costs_weighted_host`).  Nothing is computed
    here: controller by controller it is one of the two restatements.  Raises ValueError for what they refuse, naming the controller."""
    c = np.asarray(member_costs, dtype=np.float32)
    if c.ndim != 3:
        raise ValueError(f"member_costs must be (B, M, N), got {c.shape}")
    B, M, N = c.shape
    j = np.asarray(worst).reshape(-1)
    if j.size != B:
        raise ValueError(f"{j.size} values of worst for B = {B} controllers")
    with np.errstate(over="ignore"):
        rec = np.asarray(risk, dtype=np.float32)
    if rec.shape != (B, 1 + M):
        raise ValueError(f"risk must be (B, 1 + M) = ({B}, {1 + M}), got {rec.shape}")
    out = np.empty((B, N), dtype=np.float32)
    for b in range(B):
        try:
            if not 1 <= int(j[b]) <= M:  # (every controller's, weighted or not, as the library checks it)
                raise ValueError(f"worst = {j[b]} outside [1, M = {M}]")
            out[b] = aggregate_costs_host(c[b], int(j[b])) if rec[b, 0] == 0 else aggregate_costs_weighted_host(c[b], rec[b, 1:], rec[b, 0])
        except ValueError as e:
            raise ValueError(f"controller {b}: {e}") from None
    return out


def check_task(task: Task, fr3: bool = False) -> None:
    """The tasks without an ensemble plan step, refused before any model is made; raises ValueError.  `fr3`: the caller's plan step carries the arm's phase
    (judo_amd.fr3_ensemble), so fr3_pick passes."""
    if task.uses_locomotion_policy:
        raise ValueError("the Spot policy tasks have no ensemble plan step: their iteration is the materialise path (spline, policy rollout, reward, update), not one library call.  "
                         "judo_amd.spot_plants.make_spot_ensemble_controller makes the controller that keeps that path and rolls every candidate out on all the plants")
    if task.desc.get("family", task.desc["task"]) == "fr3_pick" and not fr3:
        raise ValueError("fr3_pick has no ensemble plan step: its phase is chosen per problem on the host and the ensemble entries carry none.  "
                         "judo_amd.fr3_ensemble.make_fr3_ensemble_controller makes the controller whose plan step carries the phase; one arm against perturbed "
                         "plants at the cost of a plain plan step is judo_amd.fr3_randomized.make_fr3_randomized_controller")


def _materialized_hint(why: str, fr3: bool = False) -> str:
    """`plants.materialized_hint` with this module's maker."""
    return materialized_hint(why, "ensemble", fr3)


class EnsembleController(FusedPlantController, WorstCase, Controller):
    """A `Controller` whose plan step rolls every candidate out on M plants and updates on the aggregated costs.  Everything else -- `update_states`, `action(t)`,
    `traces`, `max_opt_iters`, the three optimizers, the `none` / `min_max` normalisers, a live change of `num_rollouts` -- is the controller's own.

    `rewards` are the negated aggregated costs; `member_costs` / `member_rewards` the (M, N) costs behind them; `worst` may be set between plan steps, and
    `set_member(b, description)` replaces one plant."""

    _fr3_ensemble = False  # (FR3EnsembleController: the plan step carries the arm's phase; only an FR3EnsembleFleet takes such a member)
    _entry = "jh_plan_step_ensemble"  # the library call of the plan step: the rollout kernel on (workgroups, M), the aggregation in front of the update's tail
    _weighted_entry = "jh_plan_step_ensemble_weighted"  # ... while plant weights are set: the same rollout launch, the plant-weighted aggregation in the tail
    _a, _form, _whose, _call, _maker = "an ensemble", "ensemble", "members'", "jh_plan_step_ensemble", "ensemble"
    _member_of = "an ensemble of {}"
    _ensemble_refusal = FusedPlantController._refusal  # (the name the fleets call)

    def _check_task(self, task: Task) -> None:
        check_task(task)

    def __init__(self, controller_config: ControllerConfig, task: Task, optimizer, descriptions: Sequence[dict], worst: int | None = None,
                 device: torch.device | None = None) -> None:
        self._admit(task, descriptions)
        super().__init__(controller_config, task, optimizer, device=device)
        self._init_worst(worst, len(self._members))

    def _entry_name(self) -> str:
        """The weighted form of the call while weights are set (`set_weights`)."""
        return self._weighted_entry if self._risk_weights is not None else self._entry

    def _kind_args(self, plan, b) -> tuple:
        """The entry's arguments between K and `mode`: member_costs, costs, and `worst` or the host weights and the tail mass."""
        risk = (self._risk_weights, self.tail) if self._risk_weights is not None else (self._worst,)
        return (self._member_cost_rows(plan.shard.count).data_ptr(), _lib.ptr(b.costs), *risk)


def make_ensemble_controller(task: str | Task, optimizer: str, descriptions: Sequence[dict], worst: int | None = None, device: torch.device | None = None) -> EnsembleController:
    """`make_controller` for one controller over M plants: the registered task and optimizer (with the task's overrides) around `descriptions`, M model descriptions of
    that task (`models.scaled_description(task.desc, body_mass=..., geom_friction=..., actuator_kp=...)`).  Member 0 is the nominal plant.  `worst`: how many of a
    candidate's largest member costs are averaged; None: all M, the mean."""
    return make_for(EnsembleController, task, optimizer, descriptions, worst=worst, device=device)


__all__ = ["EnsembleController", "MAX_ENSEMBLE", "aggregate_costs_host", "aggregate_costs_risk_batch_host", "aggregate_costs_weighted_host", "check_descriptions", "check_task", "make_ensemble_controller"]
