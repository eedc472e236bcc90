"""B fr3_pick controllers planned in ONE launch (`jh_plan_step_batch_phases`, include/judo_amd.h).

fr3_pick is the one model family whose plan step takes a host decision per problem: `FR3Pick.pre_rollout` picks the phase (LIFT / MOVE / PLACE / HOMING,
judo/tasks/fr3_pick.py:191-223) from the controller's own state, and the kernel's step cost and its choice of distance sensors depend on it.  B arms are in B phases,
so `ControllerFleet` and `jh_plan_step_batch`, whose problems share every scalar argument, refuse the family.  An `FR3Fleet` is `ControllerFleet`'s loop around another
call: every member's block carries one more word behind its bounds, the member's phase as a float, and the rollout kernel on the grid (groups, B) reads its problem's word.
The reference's shipped configuration is 64 rollouts x 250 steps, a handful of one-wave workgroups per controller: eight arms fit the GPU side by side
(profiles/fr3_fleet.md has the measured sweep).

What the members share is what `ControllerFleet`'s members share, and ONE model image: a model set per problem is not available for fr3_pick, so members with perturbed
physics are refused, as is a mixture of the default and the self-collision build.  State, time, goal, seed, nominal, CEM sigma and the phase are a member's own.
Afterwards each member is bit for bit where its own `update_action()` would have left it.

An `FR3PlantFleet` lifts the one-image rule: B arms on B plants (an unknown cube mass, pad friction or gripper gain per arm) in one launch.  Its members keep a `GpuModel`
each, their images differ in the float section alone (`models.scaled_description`), and the fleet plans them through one `GpuModelSet` of fr3_pick models and
`jh_plan_step_batch_phases_models`, where problem b reads image b.  The contract is the same: member b ends bit for bit where its own `update_action()` on its own plant
would have left it, `task.phase` included.  `make_fr3_fleet(..., descriptions=[...])` makes one."""

from __future__ import annotations

from typing import Sequence

import torch

from judo_amd import _lib
from judo_amd.controller import Controller, make_controller_for
from judo_amd.device import GpuModelSet
from judo_amd.ensemble import MAX_ENSEMBLE, check_descriptions
from judo_amd.fleet import ControllerFleet, _LaunchStep, refuse_fr3_randomized
from judo_amd.models import layout
from judo_amd.tasks import FR3Pick


class FR3Fleet(ControllerFleet):
    """B fr3_pick `Controller`s of one optimizer kind whose plan steps run as one launch.  `fleet[i]` is an ordinary `Controller`: `update_states`, `optimizer.seed`,
    `action(t)`, `traces`, `rewards` and `task.phase` work per member as they do on a controller alone."""

    _fr3_members = True
    _block_extra_words = 1  # the phase word, behind the bounds
    _one_image = True  # every member plans on member 0's image (FR3PlantFleet: an image per member)

    def _check_member(self, i: int, c: Controller, first: Controller) -> None:
        refuse_fr3_randomized(i, c, self)
        if c.model is None or c.model.desc.get("family", c.model.task) != "fr3_pick" or not isinstance(c.task, FR3Pick):
            raise ValueError(f"fleet member {i} is no fr3_pick controller ({type(c.task).__name__}): an FR3Fleet plans fr3_pick alone; every other model family shares a "
                             "launch in a ControllerFleet (judo_amd.fleet.make_controller_fleet)")
        if c.task.self_collision != first.task.self_collision or c.model.self_collision != first.model.self_collision:
            raise ValueError(f"fleet member {i} differs from member 0 in self_collision: the launch runs one build of the fr3 kernel")
        if self._one_image and c.model is not first.model and c.model._blob != first.model._blob:
            raise ValueError(f"fleet member {i} has another model image than member 0: an FR3Fleet plans every member on ONE image; a model set per problem "
                             "(randomised physics) is not available for fr3_pick in this class.  An FR3PlantFleet (make_fr3_fleet(..., descriptions=...)) plans "
                             "members whose images differ in the float section alone")
        super()._check_member(i, c, first)  # (an image of a member's own: the header and the int section must be member 0's, `image_sections`, and the kernel build)

    def _models(self) -> GpuModelSet | None:
        return None  # (one image: byte-identical members were pointed at member 0's model when the fleet was made)

    def _launch(self, step: _LaunchStep) -> None:
        """The members' phases (decided by their `pre_rollout` in this iteration) into the phase words, then the B plan steps as one call."""
        self._write_phases(step.fb)
        self._launch_traced(_lib.lib().jh_plan_step_batch_phases, (self.model.handle, len(self.controllers)), step)


class FR3PlantFleet(FR3Fleet):
    """An `FR3Fleet` whose members plan on plants of their own: `fleet[i].model` is member i's `GpuModel`, and the images differ in the float section alone (masses,
    inertias, friction, gains).  One launch, a model image and a phase per problem.  Members that share member 0's image byte for byte share its `GpuModel`; a fleet of
    such members alone plans as an `FR3Fleet` does."""

    _one_image = False

    def _models(self) -> GpuModelSet | None:
        return ControllerFleet._models(self)  # (None while every member plans on the fleet's one model; else the set, which `GpuModelSet` makes with the fr3 constructor)

    def _launch(self, step: _LaunchStep) -> None:
        """The phase words, then the B plan steps as one call on the set: problem b on image b."""
        if step.model_set is None:
            return super()._launch(step)
        self._write_phases(step.fb)
        self._launch_traced(_lib.lib().jh_plan_step_batch_phases_models, (step.model_set.handle, len(self.controllers)), step)


def make_fr3_fleet(optimizer: str, B: int, device: torch.device | None = None, self_collision: bool = False, descriptions: Sequence[dict] | None = None) -> FR3Fleet:
    """B fr3_pick controllers with the registered optimizer (`make_controller_for(FR3Pick(self_collision), optimizer)`, B times) around ONE `GpuModel`.
    `self_collision`: every member on the self-collision build of the kernel (all 190 pairs of the MJCF) instead of the default one.

    `descriptions`: B model descriptions, one per member (`models.scaled_description(FR3Pick(self_collision).desc, body_mass=..., geom_friction=..., actuator_kp=...)`): an
    `FR3PlantFleet`, where member i's task takes `descriptions[i]` and keeps a `GpuModel` of its own.  The descriptions must pack to images that differ in the float
    section alone (`ensemble.check_descriptions`) and carry the `self_collision` key of the build asked for."""
    if B < 1:
        raise ValueError("a fleet needs at least one controller")
    if descriptions is not None:
        descriptions = list(descriptions)
        if len(descriptions) != B:
            raise ValueError(f"{len(descriptions)} descriptions for a fleet of {B}")
        for i, d in enumerate(descriptions):
            if d.get("family", d.get("task")) != "fr3_pick":
                raise ValueError(f"description {i} is no fr3_pick description (task {d.get('task')!r})")
            if bool(d.get("self_collision")) != bool(self_collision):
                raise ValueError(f"description {i} differs from the fleet in self_collision: derive the descriptions from FR3Pick(self_collision={bool(self_collision)}).desc")
        for lo in range(0, B, MAX_ENSEMBLE - 1):  # (the rule has an ensemble's size limit: every chunk is held to member 0)
            check_descriptions(descriptions[:1] + descriptions[max(lo, 1) : lo + MAX_ENSEMBLE - 1])
    members: list[Controller] = []
    for i in range(B):
        t = FR3Pick(self_collision=self_collision)
        if descriptions is not None:
            t.desc = descriptions[i]
            t._layout, t._ctrlrange, t._jadr = layout(t.desc), None, None
            if members and t.desc is members[0].task.desc:
                t._gpu = members[0].model
        elif members:
            t._gpu = members[0].model  # (Task.gpu_model hands it out instead of packing and uploading the image again)
        members.append(make_controller_for(t, optimizer, device=device))
    return FR3PlantFleet(members) if descriptions is not None else FR3Fleet(members)


__all__ = ["FR3Fleet", "FR3PlantFleet", "make_fr3_fleet"]
