"""One controller whose candidates are each rolled out on ONE plant of a set (`jh_plan_step_randomized`, include/judo_amd.h): domain-randomised MPPI / CEM / PS.

An `EnsembleController` rolls every candidate out on all M plants and pays M times the rollouts of a plain plan step.  A `RandomizedController` pays what a plain plan
step pays: ONE nominal spline, N candidates in G contiguous blocks of N / G rollouts, block g on plant `assignment[g]` of a `GpuModelSet`, and the update on the N costs
as they are -- the plan is never fitted to one plant.  G may exceed M: a plant named by several blocks carries that share of the candidates, which is how weights are
expressed (`blocks_from_weights`).  The assignment travels in the kernel arguments, so a new one for the next plan step costs no copy and no launch.  The reference has
no counterpart.

Member 0 is the nominal plant: the controller's `model`, on which the traces are re-rolled."""

from __future__ import annotations

import ctypes as C
from typing import Sequence

import numpy as np
import torch

from judo_amd import _lib
from judo_amd.config import ControllerConfig
from judo_amd.controller import Controller, _PlanBuffers
from judo_amd.device import GpuModel, GpuModelSet
from judo_amd.distributed import Shard
from judo_amd.ensemble import check_descriptions
from judo_amd.models import layout
from judo_amd.optimizers import get_registered_optimizers
from judo_amd.tasks import Task, get_registered_tasks

MAX_PLANT_BLOCKS = _lib.MAX_PLANT_BLOCKS


def blocks_from_weights(weights: Sequence[float], blocks: int) -> list[int]:
    """The assignment of `blocks` rollout blocks to M plants in proportion to `weights`, M non-negative numbers with a positive sum, by largest-remainder
    apportionment: plant m first gets floor(blocks * w[m] / sum(w)) blocks, and the blocks still open go one each to the plants with the largest remainders, ties to
    the lower index.  A zero weight gets no block.  The blocks of one plant are adjacent, plants in rising order: [0, 0, 0, 1, 1, 2].  A pure host function."""
    w = np.asarray(weights, dtype=np.float64).reshape(-1)
    G = int(blocks)
    if w.size < 1 or not np.isfinite(w).all() or (w < 0).any() or w.sum() <= 0:
        raise ValueError(f"weights must be non-negative, finite numbers with a positive sum, got {list(np.asarray(weights).reshape(-1))}")
    if G < 1:
        raise ValueError(f"blocks = {blocks} must be at least 1")
    quota = np.round(G * w / w.sum(), 9)  # (rounded: 10 * 0.3 / 1.0 is 3.0000000000000004, and equal weights must tie exactly)
    counts = np.floor(quota).astype(np.int64)
    rem = np.round(quota - counts, 9)  # (5.6 - 5 and 1.6 - 1 differ in the last bit and tie all the same)
    rem[w == 0] = -1.0  # (never a block for a zero weight: their quota is 0 and the positive weights' remainders add up to the open blocks)
    for m in sorted(range(w.size), key=lambda m: (-rem[m], m))[: G - int(counts.sum())]:
        counts[m] += 1
    return [m for m in range(w.size) for _ in range(int(counts[m]))]


def check_assignment(assignment: Sequence[int], members: int) -> list[int]:
    """`assignment` as a list of G plant indices, 1 <= G <= MAX_PLANT_BLOCKS, each in [0, members); raises ValueError naming the block."""
    a = [int(p) for p in assignment]
    if not 1 <= len(a) <= MAX_PLANT_BLOCKS:
        raise ValueError(f"an assignment of {len(a)} blocks is outside [1, {MAX_PLANT_BLOCKS}] (include/judo_amd.h JH_MAX_PLANT_BLOCKS)")
    for g, (p, raw) in enumerate(zip(a, assignment)):
        if p != raw or not 0 <= p < members:
            raise ValueError(f"assignment[{g}] = {raw!r} outside [0, M = {members}): block {g} names no plant of the set")
    return a


def plant_of_rollout(assignment: Sequence[int], num_rollouts: int) -> np.ndarray:
    """(N,) ints: the plant of every rollout -- block g is rollouts [g * N / G, (g + 1) * N / G).  Raises ValueError when G does not divide N."""
    G, N = len(assignment), int(num_rollouts)
    if G < 1 or N % G != 0:
        raise ValueError(f"num_rollouts % blocks != 0: {N} rollouts do not split into {G} equal blocks")
    return np.repeat(np.asarray(assignment, dtype=np.int64), N // G)


def check_task(task: Task, fr3: bool = False) -> None:
    """The tasks without a randomised plan step, refused before any model is made; raises ValueError.  `fr3`: the caller's plan step carries the arm's phase
    (judo_amd.fr3_randomized), so fr3_pick passes."""
    if task.uses_locomotion_policy:
        raise ValueError("the Spot policy tasks have no randomised plan step: their iteration is the materialise path (spline, policy rollout, reward, update), not one library call.  "
                         "judo_amd.spot_plants.make_spot_randomized_controller makes the controller that keeps that path and spreads the candidates over the plants")
    if task.desc.get("family", task.desc["task"]) == "fr3_pick" and not fr3:
        raise ValueError("fr3_pick has no randomised plan step behind this class: its phase is chosen per problem on the host, and jh_plan_step_randomized carries none.  "
                         "judo_amd.fr3_randomized.make_fr3_randomized_controller makes the controller whose plan step carries the phase, "
                         "judo_amd.fr3_randomized_fleet.make_fr3_randomized_fleet a fleet of them")


def _materialized_hint(why: str, fr3: bool = False) -> str:
    """What serves a configuration this class refuses, behind the refusal: the controller of judo_amd.materialized keeps the materialise path (a plugin reward, hook or
    optimizer, the running normaliser, more knots than the fused kernel holds) and rolls it out on the plants.  It has no sharded form and writes no candidate knots either."""
    if fr3 or "sharded path" in why or "keep_candidates" in why:  # (fr3_pick has no materialise launch on plants)
        return ""
    return ".  judo_amd.materialized.make_materialized_randomized_controller makes the controller that materialises the rollouts on the plants and scores them with Task.reward"


class RandomizedController(Controller):
    """A `Controller` whose plan step rolls block g of its candidates out on plant `assignment[g]` and updates on the N costs.  Everything else -- `update_states`,
    `action(t)`, `traces`, `max_opt_iters`, the three optimizers, the `none` / `min_max` normalisers -- is the controller's own.

    `assignment` (G plant indices, default g % M) may be set between plan steps; `plant_of_rollout` and `plant_rewards()` say which plant a reward belongs to, and
    `set_member(b, description)` replaces one plant."""

    _fr3_randomized = False  # (FR3RandomizedController: the plan step carries the arm's phase; only an FR3RandomizedFleet takes such a member)
    _entry = "jh_plan_step_randomized"  # the library call of the plan step

    def _check_task(self, task: Task) -> None:
        check_task(task)

    def _entry_args(self, W, N: int, H: int, K: int) -> tuple:
        """The entry's arguments between the noise pitch and the table: W, N, H, K."""
        return (_lib.ptr(W), N, H, K)

    def __init__(self, controller_config: ControllerConfig, task: Task, optimizer, descriptions: Sequence[dict], blocks: int | None = None,
                 weights: Sequence[float] | None = None, device: torch.device | None = None) -> None:
        self._check_task(task)
        check_descriptions(descriptions)
        self._descriptions = list(descriptions)
        M = len(self._descriptions)
        G = M if blocks is None else int(blocks)
        if weights is not None and len(weights) != M:
            raise ValueError(f"{len(weights)} weights for M = {M} plants")
        assignment = check_assignment(blocks_from_weights(weights, G) if weights is not None else [g % M for g in range(max(G, 0))], M)
        task.desc = self._descriptions[0]
        task._layout, task._ctrlrange, task._jadr, task._gpu = layout(task.desc), None, None, None
        super().__init__(controller_config, task, optimizer, device=device)
        self._members = [self.model] + [GpuModel(d, self.device) for d in self._descriptions[1:]]
        self.model_set = GpuModelSet(self._members)
        self._assignment = assignment
        self._assignment_used: list[int] | None = None  # the assignment of the last plan step: what `rewards` were rolled out on

    # ---- the plants --------------------------------------------------------------------------------------------------------------------------------
    @property
    def descriptions(self) -> list[dict]:
        return list(self._descriptions)

    @property
    def num_members(self) -> int:
        return len(self._members)

    @property
    def blocks(self) -> int:
        return len(self._assignment)

    @property
    def assignment(self) -> list[int]:
        """The plant of every rollout block, G indices in [0, M), validated when set.  Setting it takes effect at the next plan step and costs nothing on the device;
        `update_action` raises ValueError if the G blocks do not divide `num_rollouts` then."""
        return list(self._assignment)

    @assignment.setter
    def assignment(self, a: Sequence[int]) -> None:
        self._assignment = check_assignment(a, len(self._members))  # (whether the blocks divide num_rollouts, a live setting, is the plan step's check)

    def set_weights(self, weights: Sequence[float], blocks: int | None = None) -> None:
        """`assignment = blocks_from_weights(weights, blocks)`; `blocks` None keeps the number of blocks."""
        if len(weights) != len(self._members):
            raise ValueError(f"{len(weights)} weights for M = {len(self._members)} plants")
        self.assignment = blocks_from_weights(weights, len(self._assignment) if blocks is None else blocks)

    @property
    def plant_of_rollout(self) -> np.ndarray:
        """(N,) ints: the plant every rollout of the last plan step ran on (of the next one, before the first)."""
        if self._assignment_used is None:
            return plant_of_rollout(self._assignment, self.optimizer.num_rollouts)
        return plant_of_rollout(self._assignment_used, int(self.costs_device.numel()))

    def plant_rewards(self) -> np.ndarray:
        """(M,) fp64: the mean of `rewards` over the rollouts of every plant, NaN for a plant with no block."""
        r, plant = np.asarray(self.rewards, dtype=np.float64), self.plant_of_rollout
        return np.array([r[plant == m].mean() if (plant == m).any() else np.nan for m in range(len(self._members))])

    def set_member(self, b: int, description: dict) -> None:
        """Replace member b's plant (`GpuModelSet.update`: the library's checks; synchronous -- between plan steps).  b = 0 replaces the nominal plant too."""
        b = int(b)
        if not 0 <= b < len(self._members):
            raise ValueError(f"member {b} of a set of {len(self._members)} plants")
        trial = list(self._descriptions)
        trial[b] = description
        check_descriptions(trial)
        model = GpuModel(description, self.device)
        self.model_set.update(b, model)
        self._members[b], self._descriptions[b] = model, description
        if b == 0:
            self.task.desc, self.task._gpu = description, model
            self.task._layout, self.task._ctrlrange, self.task._jadr = layout(description), None, None
            self.model = self.rollout_backend.model = model

    # ---- the plan step -----------------------------------------------------------------------------------------------------------------------------
    def _hint(self, why: str) -> str:
        """What a refusal of the one-call shape adds: the maker that serves the configuration (`FR3RandomizedController` names the arm's)."""
        return _materialized_hint(why, self._fr3_randomized)

    def _randomized_refusal(self, world: int, nrm) -> str | None:
        """Why this controller's iteration is not the one-call shape, or None."""
        if world > 1 or self.force_shard_path:
            return "a process group or force_shard_path: the sharded path has no randomised form"
        if nrm.needs_moments:
            return "the running normaliser: its moments need the materialise path"
        if self.keep_candidates:
            return "keep_candidates: the randomised launch writes no candidate knots"
        if self.model is not None and self.optimizer.num_nodes > self.model.max_fused_knots_at(self.num_timesteps):
            return f"num_nodes = {self.optimizer.num_nodes} above the fused kernel's limit of {self.model.max_fused_knots_at(self.num_timesteps)} knots at this horizon (max_fused_knots_at)"
        if not self.uses_fused_cost or not (self.fused_update and hasattr(self.optimizer, "fused_update_args")):
            return "a plugin reward, hook or optimizer (uses_fused_cost is false): the plants' costs come from the fused kernels alone"
        return None

    def _iteration_shape(self, world: int, nrm) -> str:
        why = self._randomized_refusal(world, nrm)
        if why is not None:
            raise ValueError(f"a randomised controller runs its iteration as one jh_plan_step_randomized call, which this configuration rules out ({why})" + self._hint(why))
        return "plan_step"

    def update_action(self) -> None:
        if not self.uses_fused_optimizer:
            raise ValueError("a randomised controller runs its iteration as one jh_plan_step_randomized call, which this configuration rules out "
                             "(a plugin reward, hook or optimizer (uses_fused_cost is false): the plants' costs come from the fused kernels alone)" + self._hint(""))
        if self.optimizer_cfg.num_rollouts > 0 and self.optimizer_cfg.num_rollouts % len(self._assignment) != 0:  # (a live change of num_rollouts)
            raise ValueError(f"num_rollouts % blocks != 0: {self.optimizer_cfg.num_rollouts} rollouts do not split into {len(self._assignment)} equal blocks")
        super().update_action()

    def _plan_step(self, lib, b: _PlanBuffers, shape: str, noise_p: int, ldn: int, knots_out, W, shard: Shard, world: int, H: int, K: int, nu: int, stream,
                   state: dict) -> int:
        """Shape "plan_step" on the set: one upload (or the host block read in place), the batched rollout kernel on (workgroups of N / G rollouts, G), the single
        call's tail, one completion mark.  No trace buffer: the trace elites' knots are staged and re-rolled on member 0 when the traces are read."""
        opt = self.optimizer
        N, a = shard.count, self._assignment
        state["trace_buf"] = None
        b.size_out(2 * K * nu)
        mode, lam, k_el, tie = opt.fused_update_args()
        evs = [self._timing_event() for _ in range(3)] if self.record_kernel_events else None
        timing = (C.c_void_p * 3)(*[e.handle for e in evs]) if evs else None
        off = b.offsets
        in_place = b.blk_stale = self.model.closed_form
        mark = b.done_ptr if self.model.closed_form else b.out_host_ptr
        table = (C.c_ubyte * len(a))(*a)
        st = getattr(lib, self._entry)(self.model_set.handle, b.host_ptr if in_place else b.blk.data_ptr(), b.host_ptr, b.nblk_bytes, int(off[1]), int(off[2]), int(off[3]), int(off[4]),
                                       noise_p, ldn, *self._entry_args(W, N, H, K), table, len(a), _lib.ptr(b.costs), mode, lam, k_el, tie, _lib.ptr(b.fused_scratch), b.out_host_ptr, mark,
                                       timing, stream)
        _lib.check(st, self._entry)
        self._assignment_used = list(a)
        state["costs"] = b.costs
        if evs:
            self.kernel_events.append((evs[0], evs[1]))
            self.exchange_events.append((evs[1], evs[2]))
        self._fetch(b, begun=True)
        if state.get("stage") is not None:
            state["stage"]()
        return 0


def make_randomized_controller(task: str | Task, optimizer: str, descriptions: Sequence[dict], blocks: int | None = None, weights: Sequence[float] | None = None,
                               device: torch.device | None = None) -> RandomizedController:
    """`make_controller` for one controller whose candidates are spread over M plants: the registered task and optimizer (with the task's overrides) around
    `descriptions`, M model descriptions of that task (`models.scaled_description(task.desc, body_mass=..., geom_friction=..., actuator_kp=...)`).  Member 0 is the
    nominal plant.  `blocks`: the number G of rollout blocks, None: M; `weights`: M non-negative numbers that `blocks_from_weights` turns into the assignment, None:
    block g on plant g % M."""
    tasks, opts = get_registered_tasks(), get_registered_optimizers()
    if isinstance(task, str):
        if task not in tasks:
            raise ValueError(f"Task {task} not found in task registry.")
        task = tasks[task][0]()
    if optimizer not in opts:
        raise ValueError(f"Optimizer {optimizer} not found in optimizer registry.")
    opt_cls, opt_cfg_cls = opts[optimizer]
    opt_cfg = opt_cfg_cls()
    opt_cfg.set_override(task.name)
    ctrl_cfg = ControllerConfig()
    ctrl_cfg.set_override(task.name)
    return RandomizedController(ctrl_cfg, task, opt_cls(opt_cfg, task.nu), descriptions, blocks=blocks, weights=weights, device=device)


__all__ = ["MAX_PLANT_BLOCKS", "RandomizedController", "blocks_from_weights", "check_assignment", "check_task", "make_randomized_controller", "plant_of_rollout"]
