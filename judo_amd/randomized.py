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

import torch

from judo_amd import _lib
from judo_amd.config import ControllerConfig
from judo_amd.controller import Controller
from judo_amd.plants import MAX_PLANT_BLOCKS, Assignment, FusedPlantController, blocks_from_weights, check_assignment, make_for, materialized_hint, plant_of_rollout
from judo_amd.tasks import Task


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
    """`plants.materialized_hint` with this module's maker."""
    return materialized_hint(why, "randomized", fr3)


class RandomizedController(FusedPlantController, Assignment, Controller):
    """A `Controller` whose plan step rolls block g of its candidates out on plant `assignment[g]` and updates on the N costs.  Everything else -- `update_states`,
    `action(t)`, `traces`, `max_opt_iters`, the three optimizers, the `none` / `min_max` normalisers -- is the controller's own.

    `assignment` (G plant indices, default g % M) may be set between plan steps; `plant_of_rollout` and `plant_rewards()` say which plant a reward belongs to, and
    `set_member(b, description)` replaces one plant."""

    _fr3_randomized = False  # (FR3RandomizedController: the plan step carries the arm's phase; only an FR3RandomizedFleet takes such a member)
    _entry = "jh_plan_step_randomized"  # the library call of the plan step: the rollout kernel on (workgroups of N / G rollouts, G), the single call's tail
    _a, _form, _whose, _call, _maker = "a randomised", "randomised", "plants'", "jh_plan_step_randomized", "randomized"
    _randomized_refusal = FusedPlantController._refusal  # (the name the fleets call)

    def _check_task(self, task: Task) -> None:
        check_task(task)

    def __init__(self, controller_config: ControllerConfig, task: Task, optimizer, descriptions: Sequence[dict], blocks: int | None = None,
                 weights: Sequence[float] | None = None, device: torch.device | None = None) -> None:
        self._init_assignment(blocks, weights, self._admit(task, descriptions))
        super().__init__(controller_config, task, optimizer, device=device)

    def _kind_args(self, plan, b) -> tuple:
        """The entry's arguments between K and `mode`: the table, G, costs."""
        a = self._assignment
        return ((C.c_ubyte * len(a))(*a), len(a), _lib.ptr(b.costs))

    def _after_call(self, kind_args: tuple) -> None:
        self._assignment_used = list(kind_args[0])  # (the table the launch took)


def make_randomized_controller(task: str | Task, optimizer: str, descriptions: Sequence[dict], blocks: int | None = None, weights: Sequence[float] | None = None,
                               device: torch.device | None = None) -> RandomizedController:
    """`make_controller` for one controller whose candidates are spread over M plants: the registered task and optimizer (with the task's overrides) around
    `descriptions`, M model descriptions of that task (`models.scaled_description(task.desc, body_mass=..., geom_friction=..., actuator_kp=...)`).  Member 0 is the
    nominal plant.  `blocks`: the number G of rollout blocks, None: M; `weights`: M non-negative numbers that `blocks_from_weights` turns into the assignment, None:
    block g on plant g % M."""
    return make_for(RandomizedController, task, optimizer, descriptions, blocks=blocks, weights=weights, device=device)


__all__ = ["MAX_PLANT_BLOCKS", "RandomizedController", "blocks_from_weights", "check_assignment", "check_task", "make_randomized_controller", "plant_of_rollout"]
