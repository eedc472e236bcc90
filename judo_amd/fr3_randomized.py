"""One fr3_pick controller whose candidates are each rolled out on ONE plant of a set (`jh_plan_step_randomized_phase`, include/judo_amd.h).

A `RandomizedController` refuses fr3_pick because its library call has no phase: `FR3Pick.pre_rollout` picks LIFT / MOVE / PLACE / HOMING from the controller's own
state before every rollout, and the kernel's step cost depends on it.  One controller has one phase, so the randomised plan step of fr3_pick is the same launch with one
more scalar: the N candidates in G contiguous blocks of N / G rollouts on the grid (workgroups, G), block g on plant `assignment[g]` of a `GpuModelSet` of fr3_pick
models, every block in the controller's phase, and the update on the N costs as they are.  It costs what a plain plan step costs.  Pick-and-place is the task where
an unknown cube mass, pad friction or gripper gain decides whether a lift succeeds.

Everything but the call is `RandomizedController`'s: `assignment`, `set_weights`, `plant_of_rollout`, `plant_rewards()`, `set_member`; member 0 is the nominal plant,
on which the traces are re-rolled.  B such controllers share a launch in an `FR3RandomizedFleet` (judo_amd.fr3_randomized_fleet), and in no other fleet."""

from __future__ import annotations

from typing import Sequence

import torch

from judo_amd import _lib
from judo_amd.config import ControllerConfig
from judo_amd.fr3_ensemble import check_self_collision, materialized_hint
from judo_amd.plants import make_for
from judo_amd.randomized import RandomizedController, check_task
from judo_amd.tasks import FR3Pick, Task


class FR3RandomizedController(RandomizedController):
    """A `RandomizedController` of an `FR3Pick` task.  `descriptions` derive from the task's own (`models.scaled_description(task.desc, ...)`), so they carry the
    `self_collision` key of its build."""

    _fr3_randomized = True
    _entry = "jh_plan_step_randomized_phase"

    def _check_task(self, task: Task) -> None:
        check_task(task, fr3=True)  # (every line but fr3_pick's)
        if not isinstance(task, FR3Pick):
            raise ValueError(f"an FR3RandomizedController plans fr3_pick alone ({type(task).__name__}): every other model family has its randomised plan step in a "
                             "RandomizedController (judo_amd.randomized.make_randomized_controller)")

    def __init__(self, controller_config: ControllerConfig, task: Task, optimizer, descriptions: Sequence[dict], blocks: int | None = None,
                 weights: Sequence[float] | None = None, device: torch.device | None = None) -> None:
        self._check_task(task)
        check_self_collision(descriptions, task.self_collision)
        super().__init__(controller_config, task, optimizer, descriptions, blocks=blocks, weights=weights, device=device)

    def _hint(self, why: str) -> str:
        return materialized_hint(why, "randomized")

    def _entry_args(self, plan, b) -> tuple:
        return (_lib.ptr(plan.W), int(self.task.phase), plan.shard.count, plan.H, plan.K)  # (the phase `pre_rollout` chose in this iteration, as `Controller._plan_step` passes it to jh_plan_step)


def make_fr3_randomized_controller(optimizer: str, descriptions: Sequence[dict], blocks: int | None = None, weights: Sequence[float] | None = None,
                                   self_collision: bool = False, device: torch.device | None = None) -> FR3RandomizedController:
    """`make_randomized_controller` for fr3_pick: `FR3Pick(self_collision)` and the registered optimizer (with the task's overrides) around `descriptions`, M model
    descriptions of that task.  Member 0 is the nominal plant.  `blocks`: the number G of rollout blocks, None: M; `weights`: M non-negative numbers that
    `blocks_from_weights` turns into the assignment, None: block g on plant g % M."""
    return make_for(FR3RandomizedController, FR3Pick(self_collision=self_collision), optimizer, descriptions, blocks=blocks, weights=weights, device=device)


__all__ = ["FR3RandomizedController", "make_fr3_randomized_controller"]
