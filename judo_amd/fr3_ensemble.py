"""fr3_pick against an ensemble of plants: one controller (`jh_plan_step_ensemble_phase`) and B of them in ONE launch (`jh_plan_step_ensemble_batch_phases`,
include/judo_amd.h).

An `EnsembleController` refuses fr3_pick because its library call has no phase: `FR3Pick.pre_rollout` picks LIFT / MOVE / PLACE / HOMING from the controller's own
state before every rollout, and the kernel's step cost depends on it.  One controller has one phase, so the ensemble plan step of fr3_pick is the same launch with one
more scalar: the N candidates rolled out on every one of the M plants of a `GpuModelSet` of fr3_pick models on the grid (workgroups, M), every member in the
controller's phase, the aggregation (`worst` = 1: the worst case) and the update in the tail.  Pick-and-place is the task where an unknown cube mass, pad friction or
gripper gain decides whether a lift succeeds, and a worst-case plan step is what guards a lift against it.

Everything but the call is `EnsembleController`'s: `worst`, `set_member`, `member_costs`, `member_rewards`; member 0 is the nominal plant, on which the traces are
re-rolled in the controller's phase.

An `FR3EnsembleFleet` is `EnsembleFleet`'s loop around the call with a phase per controller: every member's block carries one more word behind its bounds, the member's
phase as a float (as in an `FR3Fleet`), and the fr3 kernel on the grid (workgroups, M, B) reads its controller's word.  Afterwards each member is bit for bit where its
own `update_action()` would have left it, `task.phase` included."""

from __future__ import annotations

from typing import Sequence

import torch

from judo_amd import _lib
from judo_amd.config import ControllerConfig
from judo_amd.ensemble import MAX_ENSEMBLE, EnsembleController, check_task
from judo_amd.ensemble_fleet import EnsembleFleet, check_fleet_descriptions, fleet_descriptions, fleet_worst
from judo_amd.optimizers import get_registered_optimizers
from judo_amd.plants import make_for
from judo_amd.tasks import FR3Pick, Task


def check_self_collision(descriptions: Sequence[dict], self_collision: bool) -> None:
    """The descriptions carry the `self_collision` key of the task's build; raises ValueError naming the first that does not."""
    for i, d in enumerate(descriptions):
        if bool(d.get("self_collision")) != bool(self_collision):
            raise ValueError(f"description {i} differs from the task in self_collision: derive the descriptions from FR3Pick(self_collision={bool(self_collision)}).desc")


def materialized_hint(why: str, kind: str) -> str:
    """What serves a configuration the fused fr3 classes refuse, behind the refusal: the controller of judo_amd.fr3_materialized keeps the materialise path (a plugin
    reward, hook or optimizer, the running normaliser, more knots than the fused kernel holds) and rolls it out on the plants.  It has no sharded form and writes no
    candidate knots either.  `kind`: "ensemble" or "randomized"."""
    if "sharded path" in why or "keep_candidates" in why:
        return ""
    return (f".  judo_amd.fr3_materialized.make_fr3_materialized_{kind}_controller makes the controller that materialises the arm's rollouts on the plants "
            "(jh_fr3_rollout_materialize_plants) and scores them with Task.reward")


class FR3EnsembleController(EnsembleController):
    """An `EnsembleController` of an `FR3Pick` task.  `descriptions` derive from the task's own (`models.scaled_description(task.desc, ...)`), so they carry the
    `self_collision` key of its build."""

    _fr3_ensemble = True
    _entry = "jh_plan_step_ensemble_phase"
    _weighted_entry = "jh_plan_step_ensemble_weighted_phase"

    def _check_task(self, task: Task) -> None:
        check_task(task, fr3=True)  # (every line but fr3_pick's)
        if not isinstance(task, FR3Pick):
            raise ValueError(f"an FR3EnsembleController plans fr3_pick alone ({type(task).__name__}): every other model family has its ensemble plan step in an "
                             "EnsembleController (judo_amd.ensemble.make_ensemble_controller)")

    def __init__(self, controller_config: ControllerConfig, task: Task, optimizer, descriptions: Sequence[dict], worst: int | None = None,
                 device: torch.device | None = None) -> None:
        self._check_task(task)
        check_self_collision(descriptions, task.self_collision)
        super().__init__(controller_config, task, optimizer, descriptions, worst=worst, device=device)

    def _hint(self, why: str) -> str:
        return materialized_hint(why, "ensemble")

    def _entry_args(self, plan, b) -> tuple:
        return (_lib.ptr(plan.W), int(self.task.phase), plan.shard.count, plan.H, plan.K)  # (the phase `pre_rollout` chose in this iteration, as `Controller._plan_step` passes it to jh_plan_step)


class FR3EnsembleFleet(EnsembleFleet):
    """B `FR3EnsembleController`s of one optimizer kind whose plan steps run as one launch.  `fleet[i]` is an ordinary `FR3EnsembleController`: `update_states`,
    `optimizer.seed`, `action(t)`, `traces`, `rewards`, `member_costs`, the `worst` setter, `set_member` and `task.phase` work per member as they do on a controller
    alone.  The plants are shared by all members or a member's own, as in an `EnsembleFleet`."""

    _fr3_members = True
    _fr3_ensemble_members = True
    _block_extra_words = 1  # the phase word, behind the bounds

    def _check_member(self, i: int, c, first) -> None:
        if not isinstance(c, FR3EnsembleController):
            raise ValueError(f"fleet member {i} is a {type(c).__name__}, not an FR3EnsembleController: an FR3EnsembleFleet plans fr3_pick ensemble controllers alone "
                             "(judo_amd.fr3_ensemble.make_fr3_ensemble_controller); every other family's share a launch in an EnsembleFleet")
        if c.task.self_collision != first.task.self_collision or c.model.self_collision != first.model.self_collision:
            raise ValueError(f"fleet member {i} differs from member 0 in self_collision: the launch runs one build of the fr3 kernel")
        super()._check_member(i, c, first)

    def _launch(self, step) -> None:
        """The members' phases (decided by their `pre_rollout` in this iteration) into the phase words, then the B ensemble plan steps as one call."""
        self._write_phases(step.fb)
        self._launch_ensemble(_lib.lib().jh_plan_step_ensemble_batch_phases, step)


def _fr3_parts(optimizer: str, self_collision: bool):
    """The controller configuration, `FR3Pick(self_collision)` and the registered optimizer, with the task's overrides: `make_for`'s three parts, unassembled."""
    return make_for(lambda *parts, device: parts, FR3Pick(self_collision=self_collision), optimizer)


def make_fr3_ensemble_controller(optimizer: str, descriptions: Sequence[dict], worst: int | None = None, self_collision: bool = False,
                                 device: torch.device | None = None) -> FR3EnsembleController:
    """`make_ensemble_controller` for fr3_pick: `FR3Pick(self_collision)` and the registered optimizer (with the task's overrides) around `descriptions`, M model
    descriptions of that task.  Member 0 is the nominal plant.  `worst`: how many of a candidate's largest member costs are averaged; None: all M, the mean."""
    return make_for(FR3EnsembleController, FR3Pick(self_collision=self_collision), optimizer, descriptions, worst=worst, device=device)


def make_fr3_ensemble_fleet(optimizer: str, B: int, descriptions: Sequence, worst=None, self_collision: bool = False, device: torch.device | None = None) -> FR3EnsembleFleet:
    """B `make_fr3_ensemble_controller`s in one fleet.  `descriptions`: M model descriptions of fr3_pick, which every member plans against, or B lists of M, a member's
    own plants; plant 0 of a list is that member's nominal plant.  `worst`: an int for every member, a list of B, or None for the mean."""
    if optimizer not in get_registered_optimizers():
        raise ValueError(f"Optimizer {optimizer} not found in optimizer registry.")
    lists = fleet_descriptions(B, descriptions)
    for i, descs in enumerate(lists):
        try:
            check_self_collision(descs, self_collision)
        except ValueError as e:
            raise ValueError(f"fleet member {i}: {e}") from None
    check_fleet_descriptions(lists)
    M = len(lists[0])
    if M > MAX_ENSEMBLE:
        raise ValueError(f"an ensemble of {M} members exceeds the {MAX_ENSEMBLE} of a launch (include/judo_amd.h JH_MAX_ENSEMBLE)")
    js = fleet_worst(B, M, worst)
    return FR3EnsembleFleet([make_fr3_ensemble_controller(optimizer, lists[i], worst=js[i], self_collision=self_collision, device=device) for i in range(B)])


__all__ = ["FR3EnsembleController", "FR3EnsembleFleet", "check_self_collision", "make_fr3_ensemble_controller", "make_fr3_ensemble_fleet"]
