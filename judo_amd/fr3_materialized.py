"""Plugin fr3_pick tasks on perturbed plants: the two controllers of judo_amd/materialized.py for the arm, whose rollouts are MATERIALISED on a `GpuModelSet` of fr3_pick
models by the cooperative arm kernel's own launch on plants (`jh_fr3_rollout_materialize_plants`, include/judo_amd.h).

`fr3_ensemble.FR3EnsembleController` and `fr3_randomized.FR3RandomizedController` are one library call per iteration and their costs come from the fused arm kernel
alone: they refuse a task with its own `Task.reward`, an overridden `post_rollout` or `task_to_sim_ctrl`, a plugin optimizer, `force_materialize`, a `num_nodes` above
`max_fused_knots_at(H)` and the running normaliser.  The two controllers here serve exactly those configurations of fr3_pick, as `MaterializedEnsembleController` and
`MaterializedRandomizedController` serve them for cartpole, cylinder_push and the leap family -- and as every fr3 form has arrived, behind classes and makers of their
own: `materialized.check_task` keeps refusing fr3_pick, and `GpuRolloutBackend.rollout_plants_device` sends an fr3 set to the arm's entry.

The classes override the admission alone.  The set, `set_member`, `worst` / `member_costs` / `member_rewards`, `assignment` / `set_weights` / `plant_of_rollout` /
`plant_rewards()`, the refusal of the sharded path and `_materialised_costs` are inherited, and so is the mark by which every fleet refuses such a member.

The phase stays the task's host decision: `FR3Pick.pre_rollout` picks LIFT / MOVE / PLACE / HOMING once per plan step from the controller's own state, and
`FR3Pick.reward` passes it to `jh_task_reward` for every member and every block.  The launch has no phase: materialise mode evaluates every distance sensor and
computes no cost.  The reference has no counterpart."""

from __future__ import annotations

from typing import Sequence

import torch

from judo_amd.ensemble import check_descriptions
from judo_amd.fr3_ensemble import check_self_collision
from judo_amd.materialized import MaterializedEnsembleController, MaterializedRandomizedController, check_task
from judo_amd.plants import make_for
from judo_amd.tasks import Task


def check_fr3_task(task: Task, kind: str = "ensemble") -> None:
    """The task's family must be fr3_pick (an `FR3Pick` or a plugin subclass of it); raises ValueError naming the maker that serves the task.  `kind`: "ensemble" or
    "randomized".  No device needed."""
    if task.uses_locomotion_policy:
        check_task(task, kind)  # (the Spot tasks: refused by name, with the maker of judo_amd.spot_plants)
    family = task.desc.get("family", task.desc["task"])
    if family != "fr3_pick":
        raise ValueError(f"a materialised fr3 {kind} controller plans fr3_pick alone ({type(task).__name__}, family {family}): its rollouts go through the cooperative arm "
                         f"kernel's entry, jh_fr3_rollout_materialize_plants.  Every other family's plugin tasks plan against perturbed plants in "
                         f"judo_amd.materialized.make_materialized_{kind}_controller")


def admit(task: Task, descriptions: Sequence[dict], kind: str) -> list[dict]:
    """The device-free admission of both classes: the task by family, then the descriptions by the plant admission of `FR3EnsembleController` and
    `FR3RandomizedController` -- every description in the task's `self_collision` build, so members mixed in it are refused, and images that differ in the float section
    alone (`ensemble.check_descriptions`)."""
    check_fr3_task(task, kind)
    check_self_collision(descriptions, bool(getattr(task, "self_collision", task.desc.get("self_collision", False))))
    check_descriptions(descriptions)
    return list(descriptions)


class FR3MaterializedEnsembleController(MaterializedEnsembleController):
    """A `MaterializedEnsembleController` of an fr3_pick task: N candidates, each rolled out on all M plants in one `jh_fr3_rollout_materialize_plants` launch, the reward
    once per member in the phase `pre_rollout` picked."""

    def _admit(self, task: Task, descriptions: Sequence[dict]) -> int:
        self._descriptions = admit(task, descriptions, self._task_kind)
        return len(self._descriptions)


class FR3MaterializedRandomizedController(MaterializedRandomizedController):
    """A `MaterializedRandomizedController` of an fr3_pick task: block g of the candidates on plant `assignment[g]` in one `jh_fr3_rollout_materialize_plants` launch, one
    reward call on the N rows in the phase `pre_rollout` picked."""

    def _admit(self, task: Task, descriptions: Sequence[dict]) -> int:
        self._descriptions = admit(task, descriptions, self._task_kind)
        return len(self._descriptions)


def make_fr3_materialized_ensemble_controller(task: str | Task, optimizer: str, descriptions: Sequence[dict], worst: int | None = None,
                                              device: torch.device | None = None) -> FR3MaterializedEnsembleController:
    """`materialized.make_materialized_ensemble_controller` for fr3_pick: the registered task ("fr3_pick") or a task instance -- `FR3Pick(self_collision=...)`, or a plugin
    subclass of `FR3Pick` with a reward or hooks of its own -- and the registered optimizer (fused or plugin, with the task's overrides) around `descriptions`, M model
    descriptions derived from the task's own (`models.scaled_description(task.desc, ...)`).  Member 0 is the nominal plant.  `worst`: how many of a candidate's largest
    member costs are averaged; None: all M, the mean."""
    return make_for(FR3MaterializedEnsembleController, task, optimizer, descriptions, worst=worst, device=device)


def make_fr3_materialized_randomized_controller(task: str | Task, optimizer: str, descriptions: Sequence[dict], blocks: int | None = None,
                                                weights: Sequence[float] | None = None, device: torch.device | None = None) -> FR3MaterializedRandomizedController:
    """`materialized.make_materialized_randomized_controller` for fr3_pick, the task as for `make_fr3_materialized_ensemble_controller`.  `blocks`: the number G of rollout
    blocks, None: M; `weights`: M non-negative numbers that `randomized.blocks_from_weights` turns into the assignment, None: block g on plant g % M.  G must divide
    `num_rollouts` at the plan step."""
    return make_for(FR3MaterializedRandomizedController, task, optimizer, descriptions, blocks=blocks, weights=weights, device=device)


__all__ = ["FR3MaterializedEnsembleController", "FR3MaterializedRandomizedController", "check_fr3_task", "make_fr3_materialized_ensemble_controller",
           "make_fr3_materialized_randomized_controller"]
