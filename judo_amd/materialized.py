"""Plugin tasks on perturbed plants: an ensemble controller and a domain-randomised controller whose rollouts are MATERIALISED on a `GpuModelSet`
(`jh_rollout_materialize_plants`, include/judo_amd.h).

`ensemble.EnsembleController` and `randomized.RandomizedController` are one library call per iteration, and their costs come from the fused rollout-and-cost kernels
alone: they refuse a task with its own `Task.reward`, an overridden `post_rollout` or `task_to_sim_ctrl`, a plugin optimizer, `force_materialize`, a `num_nodes` above
`max_fused_knots_at(H)` and the running normaliser.  The two controllers here serve exactly those configurations.  They keep the materialise chain of a plain
`Controller` -- spline -> `task_to_sim_ctrl` -> rollout -> `post_rollout` / `Task.reward` -> update -- and give the rollout a plant axis: they override
`Controller._materialised_costs` and nothing of the update, so every shape that reaches it ("update_fused" with and without the running normaliser's moments, the
candidates iteration of a plugin optimizer, numpy-only rewards) works unchanged.

  `MaterializedEnsembleController`    N candidates, each rolled out on all M plants in ONE launch of M blocks that share the (N, H, nu) controls; the reward once per
                                      member on its N rows, a risk measure over the M costs (`jh_ensemble_costs`: the mean of the `worst` largest), the ordinary update.
  `MaterializedRandomizedController`  N candidates in G blocks of N / G, block g on plant `assignment[g]`, one reward call on the N rows: the rollouts of a plain plan step.

The fused classes stay the fast path for the shipped costs.  Member 0 is the nominal plant: the controller's `model`, `last_rollout` and the traces.  Families:
cartpole, cylinder_push and the leap family; fr3_pick has the two subclasses of judo_amd/fr3_materialized.py, whose set goes through the arm's own entry.  The reference
has no counterpart."""

from __future__ import annotations

from typing import Sequence

import numpy as np
import torch

from judo_amd import _lib
from judo_amd.config import ControllerConfig
from judo_amd.controller import Controller
from judo_amd.device import GpuModel, GpuModelSet
from judo_amd.distributed import Shard
from judo_amd.ensemble import check_descriptions
from judo_amd.models import layout
from judo_amd.optimizers import get_registered_optimizers
from judo_amd.randomized import blocks_from_weights, check_assignment, plant_of_rollout
from judo_amd.tasks import Task, get_registered_tasks


def check_task(task: Task, kind: str = "ensemble") -> None:
    """The tasks without a materialise launch on plants, refused before any model is made; raises ValueError naming what serves them.  `kind`: "ensemble" or "randomized"."""
    if task.uses_locomotion_policy:
        raise ValueError(f"the Spot policy tasks roll out through the locomotion policy and the tree kernel, not through jh_rollout_materialize_plants: "
                         f"judo_amd.spot_plants.make_spot_{kind}_controller makes the controller that gives that rollout a plant axis")
    if task.desc.get("family", task.desc["task"]) == "fr3_pick":
        raise ValueError(f"fr3_pick has no materialise launch on plants: the cooperative arm kernel's batched instantiations are fused launches, and "
                         f"jh_rollout_materialize_plants refuses an fr3_pick set.  The shipped cost plans against perturbed plants in "
                         f"judo_amd.fr3_{kind}.make_fr3_{kind}_controller; a plugin fr3_pick task (its own reward or hooks, a plugin optimizer, the running normaliser) "
                         f"plans against them in judo_amd.fr3_materialized.make_fr3_materialized_{kind}_controller, whose rollouts go through the arm's own entry "
                         f"(jh_fr3_rollout_materialize_plants)")


class _MaterializedPlantController(Controller):
    """What the two controllers share: the admission of task and descriptions, the `GpuModelSet`, `set_member`, the materialise path whatever the task, the refusal of
    the sharded path."""

    _materialized_plants = True  # (the fleets refuse such a member by name: fleet.refuse_fr3_randomized)
    _kind = "plant"  # for messages
    _task_kind = "ensemble"

    def _admit(self, task: Task, descriptions: Sequence[dict]) -> int:
        """The device-free admission, first in a subclass's constructor: the task by family, then the descriptions by `ensemble.check_descriptions`.  Returns M."""
        check_task(task, self._task_kind)
        check_descriptions(descriptions)
        self._descriptions = list(descriptions)
        return len(self._descriptions)

    def __init__(self, controller_config: ControllerConfig, task: Task, optimizer, device: torch.device | None = None) -> None:
        task.desc = self._descriptions[0]
        task._layout, task._ctrlrange, task._jadr, task._gpu = layout(task.desc), None, None, None
        super().__init__(controller_config, task, optimizer, device=device)
        self._members = [self.model] + [GpuModel(d, self.device) for d in self._descriptions[1:]]
        self.model_set = GpuModelSet(self._members)

    @property
    def descriptions(self) -> list[dict]:
        return list(self._descriptions)

    @property
    def num_members(self) -> int:
        return len(self._members)

    @property
    def uses_fused_cost(self) -> bool:
        """False whatever the task: the plants' costs come from `Task.reward` on materialised rollouts (the fused kernels' costs are `EnsembleController`'s and
        `RandomizedController`'s)."""
        return False

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

    def _refuse_shards(self, world: int) -> None:
        if world > 1 or self.force_shard_path:
            raise ValueError(f"a materialised {self._kind} controller runs its rollouts as one jh_rollout_materialize_plants call, which this configuration rules out "
                             f"(a process group or force_shard_path: the sharded path has no {self._kind} form)")

    def _iteration_shape(self, world: int, nrm) -> str:
        self._refuse_shards(world)
        return super()._iteration_shape(world, nrm)

    def _candidates_iteration(self, lib, b, nrm, nominal_n, W, shard: Shard, H, K, nu, N, stream, state):
        self._refuse_shards(shard.world)
        return super()._candidates_iteration(lib, b, nrm, nominal_n, W, shard, H, K, nu, N, stream, state)

    def _spline_sim_controls(self, nom_d, noise_p, ldn: int, sig_d, lohi_d, knots_nku, W, shard: Shard, H: int, K: int, stream) -> tuple[torch.Tensor, torch.Tensor]:
        """The candidates' controls at the rollout times (`jh_spline_controls`, once) and what `task_to_sim_ctrl` makes of them (once)."""
        lib, nu = _lib.lib(), self.nu
        controls = torch.empty((shard.count, H, nu), dtype=torch.float32, device=self.device)
        st = lib.jh_spline_controls(_lib.ptr(W), _lib.ptr(knots_nku), _lib.ptr(nom_d), noise_p, ldn, _lib.ptr(sig_d), _lib.ptr(lohi_d) if knots_nku is None else None,
                                    shard.count, shard.offset, H, K, nu, _lib.ptr(controls), stream)
        _lib.check(st, "jh_spline_controls")
        return controls, torch.as_tensor(self.task.task_to_sim_ctrl(controls), device=self.device).to(torch.float32).contiguous()

    def _rollout_plants(self, table: list[int], x0_d, sim_controls: torch.Tensor, shared: bool) -> tuple[torch.Tensor, torch.Tensor]:
        rb = self.rollout_backend
        if not hasattr(rb, "rollout_plants_device"):
            raise ValueError(f"a materialised {self._kind} controller rolls out through GpuRolloutBackend.rollout_plants_device; the rollout backend assigned to it "
                             f"({type(rb).__name__}) has no plant axis")
        return rb.rollout_plants_device(self.model_set, table, x0_d, sim_controls, shared_controls=shared)


class MaterializedEnsembleController(_MaterializedPlantController):
    """A `Controller` on the materialise path whose iteration rolls every candidate out on M plants and updates on the aggregated costs.  `rewards` are the negated
    aggregated costs; `member_costs` / `member_rewards` the (M, N) costs behind them; `worst` may be set between plan steps, and `set_member(b, description)` replaces
    one plant.  `post_rollout` and `reward` run once per member, on that member's N rows."""

    _kind = "ensemble"
    _task_kind = "ensemble"

    def __init__(self, controller_config: ControllerConfig, task: Task, optimizer, descriptions: Sequence[dict], worst: int | None = None,
                 device: torch.device | None = None) -> None:
        M = self._admit(task, descriptions)
        if worst is not None and not 1 <= int(worst) <= M:
            raise ValueError(f"worst = {worst} outside [1, M = {M}]")
        self._worst = M if worst is None else int(worst)
        self._member_costs: torch.Tensor | None = None
        super().__init__(controller_config, task, optimizer, device=device)

    @property
    def worst(self) -> int:
        """How many of a rollout's largest member costs are averaged: 1 = the worst case, M = the mean."""
        return self._worst

    @worst.setter
    def worst(self, j: int) -> None:
        if not 1 <= int(j) <= len(self._descriptions):
            raise ValueError(f"worst = {j} outside [1, M = {len(self._descriptions)}]")
        self._worst = int(j)

    @property
    def member_costs(self) -> np.ndarray:
        """(M, N) fp32: member m's cost of every candidate of the last iteration."""
        if self._member_costs is None:
            raise RuntimeError("member_costs needs a completed update_action()")
        return self._member_costs.cpu().numpy()

    @property
    def member_rewards(self) -> np.ndarray:
        return -self.member_costs.astype(np.float64)

    def _materialised_costs(self, x0_d, nom_d, noise_p, ldn: int, sig_d, lohi_d, knots_nku, W, shard: Shard, H: int, K: int, stream) -> torch.Tensor:
        M, N = len(self._members), shard.count
        controls, sim = self._spline_sim_controls(nom_d, noise_p, ldn, sig_d, lohi_d, knots_nku, W, shard, H, K, stream)
        states, sensors = self._rollout_plants(list(range(M)), x0_d, sim, shared=True)  # M blocks of N rows, the one (N, H, nu) controls for all of them
        if self._member_costs is None or tuple(self._member_costs.shape) != (M, N):
            self._member_costs = torch.empty((M, N), dtype=torch.float32, device=self.device)
        for m in range(M):  # the reward per member, in the shapes a plain controller gives it
            self._score_rollout(states[m * N : (m + 1) * N], sensors[m * N : (m + 1) * N], controls, out=self._member_costs[m])
        self.last_rollout = (states[:N], sensors[:N], controls)  # member 0, the nominal plant
        costs = torch.empty(N, dtype=torch.float32, device=self.device)
        _lib.check(_lib.lib().jh_ensemble_costs(_lib.ptr(self._member_costs), M, N, N, self._worst, _lib.ptr(costs), stream), "jh_ensemble_costs")
        return costs


class MaterializedRandomizedController(_MaterializedPlantController):
    """A `Controller` on the materialise path whose iteration rolls block g of its candidates out on plant `assignment[g]` and updates on the N costs as they are.
    `assignment` (G plant indices, default g % M) may be set between plan steps -- it travels in the kernel arguments; `plant_of_rollout` and `plant_rewards()` say
    which plant a reward belongs to, and `set_member(b, description)` replaces one plant.  `post_rollout` and `reward` run once, on the N rows."""

    _kind = "randomised"
    _task_kind = "randomized"

    def __init__(self, controller_config: ControllerConfig, task: Task, optimizer, descriptions: Sequence[dict], blocks: int | None = None,
                 weights: Sequence[float] | None = None, device: torch.device | None = None) -> None:
        M = self._admit(task, descriptions)
        G = M if blocks is None else int(blocks)
        if weights is not None and len(weights) != M:
            raise ValueError(f"{len(weights)} weights for M = {M} plants")
        self._assignment = check_assignment(blocks_from_weights(weights, G) if weights is not None else [g % M for g in range(max(G, 0))], M)
        self._assignment_used: list[int] | None = None  # the assignment of the last plan step: what `rewards` were rolled out on
        super().__init__(controller_config, task, optimizer, device=device)

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
        self._assignment = check_assignment(a, len(self._descriptions))

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

    def _materialised_costs(self, x0_d, nom_d, noise_p, ldn: int, sig_d, lohi_d, knots_nku, W, shard: Shard, H: int, K: int, stream) -> torch.Tensor:
        a = list(self._assignment)
        controls, sim = self._spline_sim_controls(nom_d, noise_p, ldn, sig_d, lohi_d, knots_nku, W, shard, H, K, stream)
        states, sensors = self._rollout_plants(a, x0_d, sim, shared=False)  # G blocks of N / G rows, each on its own rows of the controls
        self._assignment_used = a
        return self._score_rollout(states, sensors, controls)


def _make(cls, task: str | Task, optimizer: str, descriptions: Sequence[dict], device, **kw):
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
    return cls(ctrl_cfg, task, opt_cls(opt_cfg, task.nu), descriptions, device=device, **kw)


def make_materialized_ensemble_controller(task: str | Task, optimizer: str, descriptions: Sequence[dict], worst: int | None = None,
                                          device: torch.device | None = None) -> MaterializedEnsembleController:
    """`make_controller` for one controller on the materialise path over M plants: the registered task (or a task instance: a plugin with its own reward or hooks) and
    the registered optimizer (fused or plugin, with the task's overrides) around `descriptions`, M model descriptions of the task's model
    (`models.scaled_description(task.desc, body_mass=..., geom_friction=..., actuator_kp=...)`).  Member 0 is the nominal plant.  `worst`: how many of a candidate's
    largest member costs are averaged; None: all M, the mean."""
    return _make(MaterializedEnsembleController, task, optimizer, descriptions, device, worst=worst)


def make_materialized_randomized_controller(task: str | Task, optimizer: str, descriptions: Sequence[dict], blocks: int | None = None,
                                            weights: Sequence[float] | None = None, device: torch.device | None = None) -> MaterializedRandomizedController:
    """`make_controller` for one controller on the materialise path whose candidates are spread over M plants.  `blocks`: the number G of rollout blocks, None: M;
    `weights`: M non-negative numbers that `randomized.blocks_from_weights` turns into the assignment, None: block g on plant g % M.  G must divide `num_rollouts` at
    the plan step."""
    return _make(MaterializedRandomizedController, task, optimizer, descriptions, device, blocks=blocks, weights=weights)


__all__ = ["MaterializedEnsembleController", "MaterializedRandomizedController", "check_task", "make_materialized_ensemble_controller",
           "make_materialized_randomized_controller"]
