"""The plant axis of the controllers, in one place: what every controller over a set of perturbed plants shares, whichever call stands behind its iteration.

The classes of judo_amd/ensemble.py, randomized.py, materialized.py and spot_plants.py are assembled from the plain mix-ins here, in front of `Controller`:

  `PlantSet`             the M descriptions, member 0 as the nominal plant, `set_member`; `GpuPlantSet` is the one over a `GpuModelSet` (`jh_model_set_create`),
                         `spot_plants._SpotPlantController` supplies the one over a `SpotPlantSet`.
  `WorstCase`            the risk measure of the ensemble controllers: `worst`, `member_costs`, `member_rewards`, the (M, N) buffer; `set_weights`, `weights`, `tail`: the plant-weighted one.
  `Assignment`           the table from rollout block to plant of the randomised controllers: `blocks`, `assignment`, `set_weights`, `plant_of_rollout`, `plant_rewards`.
  `FusedPlantController` the one-call plan step of `EnsembleController` and `RandomizedController` (`jh_plan_step_ensemble`, `jh_plan_step_randomized` and their `_phase`
                         forms: one launcher in the library, judo_amd/csrc/jh_api.hip plan_step_set), with its refusals.
  `PlantFleet`           what `EnsembleFleet` and `RandomizedFleet` add to `ControllerFleet`: every plant held to fleet member 0's plant 0, and the set of the launch.

`make_for` is the registry lookup behind every `make_*_controller`; `spline_controls` the `jh_spline_controls` call of the materialise paths (controller.py's).  The host
functions of the admission (`check_descriptions`, `check_assignment`, `blocks_from_weights`, `plant_of_rollout`) live here and stay importable from ensemble.py and randomized.py."""

from __future__ import annotations

import ctypes as C
from typing import Sequence

import numpy as np
import torch

from judo_amd import _lib
from judo_amd.config import ControllerConfig
from judo_amd.controller import _IterState, _Plan, _PlanBuffers, spline_controls
from judo_amd.device import GpuModel, GpuModelSet
from judo_amd.models import image_sections, layout, pack_model
from judo_amd.optimizers import get_registered_optimizers
from judo_amd.tasks import Task, get_registered_tasks

MAX_ENSEMBLE = _lib.MAX_ENSEMBLE
MAX_PLANT_BLOCKS = _lib.MAX_PLANT_BLOCKS


def make_for(cls, task: str | Task, optimizer: str, *args, device: torch.device | None = None, **kw):
    """`cls(controller config, task, optimizer, *args, device=device, **kw)` from the registries: the registered task (or a task INSTANCE, one built with constructor
    arguments or a plugin) and the registered optimizer, both configurations with the overrides registered for the task's name."""
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
    return cls(ctrl_cfg, task, opt_cls(opt_cfg, task.nu), *args, device=device, **kw)


# ---- the admission, without a device -----------------------------------------------------------------------------------------------------------------------
def check_descriptions(descriptions: Sequence[dict]) -> list[bytes]:
    """The admission rule of an ensemble, without a device (the rule `ControllerFleet` applies to members with images of their own): the descriptions pack to images
    whose header and int section are member 0's byte for byte -- the float section alone may differ (masses, inertias, friction, gains: `models.scaled_description`).
    Returns the packed images; raises ValueError naming the member and the section."""
    if len(descriptions) < 1:
        raise ValueError("an ensemble needs at least one description")
    if len(descriptions) > MAX_ENSEMBLE:
        raise ValueError(f"an ensemble of {len(descriptions)} members exceeds the {MAX_ENSEMBLE} of a launch (include/judo_amd.h JH_MAX_ENSEMBLE)")
    blobs = [bytes(pack_model(d)) for d in descriptions]
    want = image_sections(blobs[0])
    for i, blob in enumerate(blobs[1:], start=1):
        if blob == blobs[0]:
            continue
        for name, x, y in zip(("header", "float section", "int section"), image_sections(blob), want):
            if (x != y and name != "float section") or len(x) != len(y):
                raise ValueError(f"ensemble member {i} has another model image than member 0: the {name} of its image differs")
    return blobs


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


def materialized_hint(why: str, kind: str, fr3: bool = False) -> str:
    """What serves a configuration a fused class refuses, behind the refusal: the controller of judo_amd.materialized keeps the materialise path (a plugin reward, hook or
    optimizer, the running normaliser, more knots than the fused kernel holds) and rolls it out on the plants.  It has no sharded form and writes no candidate knots
    either.  `kind`: "ensemble" or "randomized"."""
    if fr3 or "sharded path" in why or "keep_candidates" in why:  # (fr3_pick has no materialise launch on plants)
        return ""
    return f".  judo_amd.materialized.make_materialized_{kind}_controller makes the controller that materialises the rollouts on the plants and scores them with Task.reward"


# ---- the set ---------------------------------------------------------------------------------------------------------------------------------------------------
def _relayout(task: Task, description: dict) -> None:
    """`description` becomes the task's model: the nominal plant's."""
    task.desc = description
    task._layout, task._ctrlrange, task._jadr = layout(description), None, None


class PlantSet:
    """A controller over M plants, in front of `Controller` in a class's bases.  The subclass's constructor admits the descriptions into `_descriptions` without a device
    and then calls this one, which makes the controller on member 0, the nominal plant, and then the set (`_make_set`).  `_replace_plant(b, description)` is the
    set's own step of `set_member`."""

    _member_of = "a set of {} plants"  # for `set_member`'s message

    def __init__(self, controller_config: ControllerConfig, task: Task, optimizer, device: torch.device | None = None) -> None:
        _relayout(task, self._descriptions[0])
        task._gpu = None
        super().__init__(controller_config, task, optimizer, device=device)
        self._make_set()

    @property
    def descriptions(self) -> list[dict]:
        return list(self._descriptions)

    @property
    def num_members(self) -> int:
        return len(self._descriptions)

    def set_member(self, b: int, description: dict) -> None:
        """Replace member b's plant (the set's `update` / `set_member`: the library's checks; synchronous -- between plan steps).  b = 0 replaces the nominal plant too."""
        b = int(b)
        if not 0 <= b < len(self._descriptions):
            raise ValueError(f"member {b} of " + self._member_of.format(len(self._descriptions)))
        self._replace_plant(b, description)
        self._descriptions[b] = description
        if b == 0:
            _relayout(self.task, description)


class GpuPlantSet(PlantSet):
    """The plants as `GpuModel`s in a `GpuModelSet`: `_members` (member 0 is the controller's `model`) and `model_set`.  `_check_task(task)` is the subclass's."""

    def _admit(self, task: Task, descriptions: Sequence[dict]) -> int:
        """The device-free admission, first in a subclass's constructor: the task by family, then the descriptions by `check_descriptions`.  Returns M."""
        self._check_task(task)
        check_descriptions(descriptions)
        self._descriptions = list(descriptions)
        return len(self._descriptions)

    def _make_set(self) -> None:
        self._members = [self.model] + [GpuModel(d, self.device) for d in self._descriptions[1:]]
        self.model_set = GpuModelSet(self._members)

    def _replace_plant(self, b: int, description: dict) -> None:
        trial = list(self._descriptions)
        trial[b] = description
        check_descriptions(trial)
        model = GpuModel(description, self.device)
        self.model_set.update(b, model)
        self._members[b] = model
        if b == 0:
            self.task._gpu = self.model = self.rollout_backend.model = model


# ---- the two kinds -----------------------------------------------------------------------------------------------------------------------------------------------
class WorstCase:
    """The risk measure of a controller that rolls every candidate out on all M plants: a candidate's cost is the mean of the `worst` largest of its M member costs
    (`jh_plan_step_ensemble`'s tail or `jh_ensemble_costs`; `ensemble.aggregate_costs_host` restates it).  With `set_weights` it becomes the plant-weighted one, the
    tail mean of the M member costs under a probability vector (`jh_plan_step_ensemble_weighted`'s tail or `jh_ensemble_costs_weighted`;
    `ensemble.aggregate_costs_weighted_host` restates it): the weights and the tail mass travel in the kernel arguments, so new ones for the next plan step cost no
    copy and no launch."""

    _risk_weights = None  # the (JH_MAX_ENSEMBLE,) ctypes floats of the weighted measure (the first M are the weights), or None: the `worst` measure
    _risk_tail: float | None = None  # the tail mass, once set; before that `worst / M`

    def _init_worst(self, worst: int | None, M: int) -> None:
        self._worst, self._member_costs = M, None
        self._risk_weights, self._risk_tail = None, None
        if worst is not None:
            self._worst = self._checked_worst(worst, M)

    def set_weights(self, weights: Sequence[float] | None, tail: float | None = None, **assignment) -> None:
        """The plant-weighted risk measure from the next plan step on: a candidate's cost is the tail mean of its M member costs under `weights` with the tail mass
        `tail`.  `weights`: M non-negative, finite numbers with a positive sum; they are normalised in fp64 and rounded to fp32.  `tail`: in (0, 1]; None keeps the
        current one, which is `worst / M` before any was set -- uniform weights then mean what `worst` meant.  `set_weights(None)` returns to the `worst` measure (the
        tail is kept).  Validated here; raises ValueError and changes nothing.  (No controller is both a `WorstCase` and an `Assignment`; a class assembled from both
        pieces keeps `set_weights` for its assignment, with that method's keywords.)"""
        if isinstance(self, Assignment):
            return Assignment.set_weights(self, weights, **({} if tail is None else {"tail": tail}), **assignment)
        if assignment:
            raise TypeError(f"set_weights() got an unexpected keyword argument {next(iter(assignment))!r}")
        M = len(self._descriptions)
        if tail is not None:
            t = float(np.float32(tail))
            if not 0 < t <= 1:  # (false for NaN)
                raise ValueError(f"tail = {tail} outside (0, 1]")
        if weights is None:
            self._risk_weights = None
        else:
            w = np.asarray(weights, dtype=np.float64).reshape(-1)
            if w.size != M:
                raise ValueError(f"{w.size} weights for M = {M} plants")
            if not np.isfinite(w).all() or (w < 0).any() or not w.sum() > 0 or not np.isfinite(w.sum()):
                raise ValueError(f"weights must be non-negative, finite numbers with a positive sum, got {list(w)}")
            p = (w / w.sum()).astype(np.float32)
            if not (p > 0).any():
                raise ValueError(f"weights must be non-negative, finite numbers with a positive sum, got {list(w)}")
            self._risk_weights = (C.c_float * MAX_ENSEMBLE)(*p.tolist())
        if tail is not None:
            self._risk_tail = t

    @property
    def weights(self) -> np.ndarray | None:
        """None under the `worst` measure; else a copy of the M fp32 weights of the plant-weighted one."""
        if self._risk_weights is None:
            return None
        return np.array(self._risk_weights[: len(self._descriptions)], dtype=np.float32)

    @property
    def tail(self) -> float:
        """The tail mass of the plant-weighted measure: what `set_weights` set last, `worst / M` before that."""
        if self._risk_tail is not None:
            return self._risk_tail
        return float(np.float32(self._worst) / np.float32(len(self._descriptions)))

    def _aggregate(self, rows: torch.Tensor, M: int, N: int, costs: torch.Tensor, stream) -> None:
        """The aggregation alone on the (M, N) member costs of a materialise path: `jh_ensemble_costs_weighted` while weights are set, else `jh_ensemble_costs`."""
        if self._risk_weights is not None:
            _lib.check(_lib.lib().jh_ensemble_costs_weighted(_lib.ptr(rows), M, N, N, self._risk_weights, self.tail, _lib.ptr(costs), stream), "jh_ensemble_costs_weighted")
        else:
            _lib.check(_lib.lib().jh_ensemble_costs(_lib.ptr(rows), M, N, N, self._worst, _lib.ptr(costs), stream), "jh_ensemble_costs")

    @staticmethod
    def _checked_worst(j: int, M: int) -> int:
        if not 1 <= int(j) <= M:
            raise ValueError(f"worst = {j} outside [1, M = {M}]")
        return int(j)

    @property
    def worst(self) -> int:
        """How many of a rollout's largest member costs are averaged: 1 = the worst case, M = the mean."""
        return self._worst

    @worst.setter
    def worst(self, j: int) -> None:
        self._worst = self._checked_worst(j, len(self._descriptions))

    def _member_cost_rows(self, N: int) -> torch.Tensor:
        """The (M, N) device buffer the iteration writes, made anew when M or N changed."""
        M = len(self._descriptions)
        if self._member_costs is None or tuple(self._member_costs.shape) != (M, N):
            self._member_costs = torch.empty((M, N), dtype=torch.float32, device=self.device)
        return self._member_costs

    @property
    def member_costs(self) -> np.ndarray:
        """(M, N) fp32: member m's cost of every candidate of the last iteration."""
        if self._member_costs is None:
            raise RuntimeError("member_costs needs a completed update_action()")
        return self._member_costs.cpu().numpy()

    @property
    def member_rewards(self) -> np.ndarray:
        return -self.member_costs.astype(np.float64)


class Assignment:
    """The table of a controller that rolls block g of its N candidates out on plant `assignment[g]`: G blocks of N / G rollouts, default g % M.  It travels in the
    kernel arguments, so a new one for the next plan step costs no copy."""

    def _init_assignment(self, blocks: int | None, weights: Sequence[float] | None, M: int) -> None:
        G = M if blocks is None else int(blocks)
        if weights is not None and len(weights) != M:
            raise ValueError(f"{len(weights)} weights for M = {M} plants")
        self._assignment = check_assignment(blocks_from_weights(weights, G) if weights is not None else [g % max(M, 1) for g in range(max(G, 0))], M)
        self._assignment_used: list[int] | None = None  # the assignment of the last plan step: what `rewards` were rolled out on

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
        self._assignment = check_assignment(a, len(self._descriptions))  # (whether the blocks divide num_rollouts, a live setting, is the plan step's check)

    def set_weights(self, weights: Sequence[float], blocks: int | None = None) -> None:
        """`assignment = blocks_from_weights(weights, blocks)`; `blocks` None keeps the number of blocks."""
        if len(weights) != len(self._descriptions):
            raise ValueError(f"{len(weights)} weights for M = {len(self._descriptions)} plants")
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
        return np.array([r[plant == m].mean() if (plant == m).any() else np.nan for m in range(len(self._descriptions))])

    def update_action(self) -> None:
        if self.optimizer_cfg.num_rollouts > 0 and self.optimizer_cfg.num_rollouts % len(self._assignment) != 0:  # (a live change of num_rollouts)
            raise ValueError(f"num_rollouts % blocks != 0: {self.optimizer_cfg.num_rollouts} rollouts do not split into {len(self._assignment)} equal blocks")
        super().update_action()


# ---- the one-call plan step ------------------------------------------------------------------------------------------------------------------------------------
class FusedPlantController(GpuPlantSet):
    """What `EnsembleController` and `RandomizedController` share: an iteration that is ONE library call on the set (`_entry`), whose costs come from the fused rollout
    kernels alone, and the refusal of every configuration that is not.  A subclass names itself in `_a` ... `_maker`, gives the entry's arguments between K and `mode`
    (`_kind_args`) and may look at them after the call (`_after_call`); the fr3 subclasses override `_entry`, `_entry_args`, `_check_task` and `_hint`."""

    _a, _form, _whose, _call, _maker = "a plant", "plant", "plants'", "jh_plan_step", "kind"  # in messages: the controller, its form, whose costs, the call; `materialized_hint`'s kind

    def _entry_args(self, plan: _Plan, b: _PlanBuffers) -> tuple:
        """The entry's arguments between the noise pitch and `_kind_args`: W, N, H, K."""
        return (_lib.ptr(plan.W), plan.shard.count, plan.H, plan.K)

    def _hint(self, why: str) -> str:
        """What a refusal of the one-call shape adds: the maker that serves the configuration (the fr3 subclasses name the arm's)."""
        return materialized_hint(why, self._maker)

    def _refusal(self, world: int, nrm) -> str | None:
        """Why this controller's iteration is not the one-call shape, or None."""
        if world > 1 or self.force_shard_path:
            return f"a process group or force_shard_path: the sharded path has no {self._form} form"
        if nrm.needs_moments:
            return "the running normaliser: its moments need the materialise path"
        if self.keep_candidates:
            return f"keep_candidates: the {self._form} launch writes no candidate knots"
        if self.model is not None and self.optimizer.num_nodes > self.model.max_fused_knots_at(self.num_timesteps):
            return f"num_nodes = {self.optimizer.num_nodes} above the fused kernel's limit of {self.model.max_fused_knots_at(self.num_timesteps)} knots at this horizon (max_fused_knots_at)"
        if not self.uses_fused_cost or not (self.fused_update and hasattr(self.optimizer, "fused_update_args")):
            return f"a plugin reward, hook or optimizer (uses_fused_cost is false): the {self._whose} costs come from the fused kernels alone"
        return None

    def _ruled_out(self, why: str, hint_for: str) -> ValueError:
        return ValueError(f"{self._a} controller runs its iteration as one {self._call} call, which this configuration rules out ({why})" + self._hint(hint_for))

    def _iteration_shape(self, world: int, nrm) -> str:
        why = self._refusal(world, nrm)
        if why is not None:
            raise self._ruled_out(why, why)
        return "plan_step"

    def update_action(self) -> None:
        if not self.uses_fused_optimizer:
            raise self._ruled_out(f"a plugin reward, hook or optimizer (uses_fused_cost is false): the {self._whose} costs come from the fused kernels alone", "")
        super().update_action()

    def _after_call(self, kind_args: tuple) -> None:
        pass

    def _entry_name(self) -> str:
        """The library call of this plan step: `_entry`, unless a subclass's state picks another form of it."""
        return self._entry

    def _plan_step(self, plan: _Plan, b: _PlanBuffers, st: _IterState, shape: str) -> int:
        """Shape "plan_step" on the set: one upload (or the host block read in place), the batched rollout kernel with the plants on its second grid dimension, the
        update's tail, one completion mark.  No trace buffer: the trace elites' knots are staged and re-rolled on member 0 when the traces are read."""
        st.trace_buf = None
        b.size_out(2 * plan.K * plan.nu)
        kind_args = self._kind_args(plan, b)
        mode, lam, k_el, tie = self.optimizer.fused_update_args()
        evs = [self._timing_event() for _ in range(3)] if self.record_kernel_events else None
        timing = (C.c_void_p * 3)(*[e.handle for e in evs]) if evs else None
        off = b.offsets
        in_place = b.blk_stale = self.model.closed_form
        mark = b.done_ptr if self.model.closed_form else b.out_host_ptr
        entry = self._entry_name()
        rc = getattr(_lib.lib(), entry)(self.model_set.handle, b.host_ptr if in_place else b.blk.data_ptr(), b.host_ptr, b.nblk_bytes, int(off[1]), int(off[2]), int(off[3]),
                                              int(off[4]), st.noise_p, st.ldn, *self._entry_args(plan, b), *kind_args, mode, lam, k_el, tie, _lib.ptr(b.fused_scratch), b.out_host_ptr,
                                              mark, timing, st.stream)
        _lib.check(rc, entry)
        self._after_call(kind_args)
        st.costs = b.costs
        if evs:
            self.kernel_events.append((evs[0], evs[1]))
            self.exchange_events.append((evs[1], evs[2]))
        self._fetch(b, begun=True)
        if st.stages:
            self._stage_traces(plan, b, st)
        return 0


# ---- the fleets ------------------------------------------------------------------------------------------------------------------------------------------------
class PlantFleet:
    """What a fleet of controllers over plants adds to `ControllerFleet`, in front of it in the bases: every plant of every member is held to fleet member 0's plant 0, and
    the launch reads one set of M images or one of B * M."""

    _set_key: tuple = ()  # the plants `_model_set` was made from

    def _check_plants(self, i: int, c, first) -> None:
        """Every plant of member i against fleet member 0's plant 0: one structure and one kernel build for the launch."""
        want = None
        for j, m in enumerate(c._members):
            if m is first.model or m._blob == first.model._blob:
                continue
            want = want or image_sections(first.model._blob)
            for name, x, y in zip(("header", "float section", "int section"), image_sections(m._blob), want):
                if (x != y and name != "float section") or len(x) != len(y):
                    raise ValueError(f"fleet member {i}: plant {j} has another model image than member 0's plant 0: the {name} of its image differs")
            if m.build() != first.model.build() or m.self_collision != first.model.self_collision:
                raise ValueError(f"fleet member {i}: plant {j} has another kernel build than member 0's plant 0: the kernel build or the self-collision setting differs")

    def _trace_floats(self) -> int:
        return 0  # (no trace buffer, as for the members' own call: a member stages its trace elites' knots and re-rolls them on its plant 0)

    def _models(self) -> GpuModelSet:
        """The plants of the launch: member 0's M where every member's plants are byte-identical to them, list for list; else all B * M, controller-major.  Rebuilt when
        a member's plant was exchanged between plan steps (told by identity, as `ControllerFleet._models` tells it)."""
        lists = [c._members for c in self.controllers]
        key = tuple(m for plants in lists for m in plants)
        if self._model_set is not None and len(key) == len(self._set_key) and all(a is b for a, b in zip(key, self._set_key)):
            return self._model_set
        shared = all(all(a is b or a._blob == b._blob for a, b in zip(plants, lists[0])) for plants in lists[1:])
        self._model_set = GpuModelSet(list(lists[0]) if shared else list(key))
        self._set_key = key
        return self._model_set


__all__ = ["Assignment", "FusedPlantController", "GpuPlantSet", "MAX_ENSEMBLE", "MAX_PLANT_BLOCKS", "PlantFleet", "PlantSet", "WorstCase", "blocks_from_weights",
           "check_assignment", "check_descriptions", "make_for", "materialized_hint", "plant_of_rollout", "spline_controls"]
