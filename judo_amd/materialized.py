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

import torch

from judo_amd.config import ControllerConfig
from judo_amd.controller import Controller
from judo_amd.plants import Assignment, GpuPlantSet, WorstCase, make_for, spline_controls
from judo_amd.tasks import Task


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


class _MaterializedPlantController(GpuPlantSet, Controller):
    """What the two controllers share: the admission of task and descriptions, the `GpuModelSet` and `set_member` (`plants.GpuPlantSet`), the materialise path whatever
    the task, the refusal of the sharded path."""

    _materialized_plants = True  # (the fleets refuse such a member by name: fleet.refuse_fr3_randomized)
    _kind = "plant"  # for messages
    _task_kind = "ensemble"

    def _check_task(self, task: Task) -> None:
        check_task(task, self._task_kind)

    @property
    def uses_fused_cost(self) -> bool:
        """False whatever the task: the plants' costs come from `Task.reward` on materialised rollouts (the fused kernels' costs are `EnsembleController`'s and
        `RandomizedController`'s)."""
        return False

    def _sim_controls(self, controls: torch.Tensor) -> torch.Tensor:
        """What `task_to_sim_ctrl` makes of the candidates' controls (once)."""
        return torch.as_tensor(self.task.task_to_sim_ctrl(controls), device=self.device).to(torch.float32).contiguous()

    def _refuse_shards(self, world: int) -> None:
        if world > 1 or self.force_shard_path:
            raise ValueError(f"a materialised {self._kind} controller runs its rollouts as one jh_rollout_materialize_plants call, which this configuration rules out "
                             f"(a process group or force_shard_path: the sharded path has no {self._kind} form)")

    def _iteration_shape(self, world: int, nrm) -> str:
        self._refuse_shards(world)
        return super()._iteration_shape(world, nrm)

    def _candidates_iteration(self, plan, b, st) -> None:
        self._refuse_shards(plan.shard.world)
        super()._candidates_iteration(plan, b, st)

    def _rollout_plants(self, table: list[int], x0_d, sim_controls: torch.Tensor, shared: bool) -> tuple[torch.Tensor, torch.Tensor]:
        rb = self.rollout_backend
        if not hasattr(rb, "rollout_plants_device"):
            raise ValueError(f"a materialised {self._kind} controller rolls out through GpuRolloutBackend.rollout_plants_device; the rollout backend assigned to it "
                             f"({type(rb).__name__}) has no plant axis")
        return rb.rollout_plants_device(self.model_set, table, x0_d, sim_controls, shared_controls=shared)


class MaterializedEnsembleController(WorstCase, _MaterializedPlantController):
    """A `Controller` on the materialise path whose iteration rolls every candidate out on M plants and updates on the aggregated costs.  `rewards` are the negated
    aggregated costs; `member_costs` / `member_rewards` the (M, N) costs behind them; `worst` may be set between plan steps, and `set_member(b, description)` replaces
    one plant.  `post_rollout` and `reward` run once per member, on that member's N rows."""

    _kind = "ensemble"
    _task_kind = "ensemble"

    def __init__(self, controller_config: ControllerConfig, task: Task, optimizer, descriptions: Sequence[dict], worst: int | None = None,
                 device: torch.device | None = None) -> None:
        self._init_worst(worst, self._admit(task, descriptions))
        super().__init__(controller_config, task, optimizer, device=device)

    def _materialised_costs(self, plan, b, st) -> torch.Tensor:
        M, N = len(self._members), plan.shard.count
        controls = spline_controls(self, plan, b, st)
        states, sensors = self._rollout_plants(list(range(M)), b.x0, self._sim_controls(controls), shared=True)  # M blocks of N rows, the one (N, H, nu) controls for all of them
        rows = self._member_cost_rows(N)
        for m in range(M):  # the reward per member, in the shapes a plain controller gives it
            self._score_rollout(states[m * N : (m + 1) * N], sensors[m * N : (m + 1) * N], controls, out=rows[m])
        self.last_rollout = (states[:N], sensors[:N], controls)  # member 0, the nominal plant
        costs = torch.empty(N, dtype=torch.float32, device=self.device)
        self._aggregate(rows, M, N, costs, st.stream)  # (`jh_ensemble_costs`, or its weighted form while plant weights are set)
        return costs


class MaterializedRandomizedController(Assignment, _MaterializedPlantController):
    """A `Controller` on the materialise path whose iteration rolls block g of its candidates out on plant `assignment[g]` and updates on the N costs as they are.
    `assignment` (G plant indices, default g % M) may be set between plan steps -- it travels in the kernel arguments; `plant_of_rollout` and `plant_rewards()` say
    which plant a reward belongs to, and `set_member(b, description)` replaces one plant.  `post_rollout` and `reward` run once, on the N rows."""

    _kind = "randomised"
    _task_kind = "randomized"

    def __init__(self, controller_config: ControllerConfig, task: Task, optimizer, descriptions: Sequence[dict], blocks: int | None = None,
                 weights: Sequence[float] | None = None, device: torch.device | None = None) -> None:
        self._init_assignment(blocks, weights, self._admit(task, descriptions))
        super().__init__(controller_config, task, optimizer, device=device)

    def _materialised_costs(self, plan, b, st) -> torch.Tensor:
        a = list(self._assignment)
        controls = spline_controls(self, plan, b, st)
        states, sensors = self._rollout_plants(a, b.x0, self._sim_controls(controls), shared=False)  # G blocks of N / G rows, each on its own rows of the controls
        self._assignment_used = a
        return self._score_rollout(states, sensors, controls)


def make_materialized_ensemble_controller(task: str | Task, optimizer: str, descriptions: Sequence[dict], worst: int | None = None,
                                          device: torch.device | None = None) -> MaterializedEnsembleController:
    """`make_controller` for one controller on the materialise path over M plants: the registered task (or a task instance: a plugin with its own reward or hooks) and
    the registered optimizer (fused or plugin, with the task's overrides) around `descriptions`, M model descriptions of the task's model
    (`models.scaled_description(task.desc, body_mass=..., geom_friction=..., actuator_kp=...)`).  Member 0 is the nominal plant.  `worst`: how many of a candidate's
    largest member costs are averaged; None: all M, the mean."""
    return make_for(MaterializedEnsembleController, task, optimizer, descriptions, worst=worst, device=device)


def make_materialized_randomized_controller(task: str | Task, optimizer: str, descriptions: Sequence[dict], blocks: int | None = None,
                                            weights: Sequence[float] | None = None, device: torch.device | None = None) -> MaterializedRandomizedController:
    """`make_controller` for one controller on the materialise path whose candidates are spread over M plants.  `blocks`: the number G of rollout blocks, None: M;
    `weights`: M non-negative numbers that `randomized.blocks_from_weights` turns into the assignment, None: block g on plant g % M.  G must divide `num_rollouts` at
    the plan step."""
    return make_for(MaterializedRandomizedController, task, optimizer, descriptions, blocks=blocks, weights=weights, device=device)


__all__ = ["MaterializedEnsembleController", "MaterializedRandomizedController", "check_task", "make_materialized_ensemble_controller",
           "make_materialized_randomized_controller"]
