"""B domain-randomised fr3_pick controllers planned in ONE launch (`jh_plan_step_randomized_batch_phases`, include/judo_amd.h).

An `FR3RandomizedController` spreads the rollout blocks of one arm over the plants of its set and plans alone; a `RandomizedFleet` refuses it because its library call
has no phase.  An `FR3RandomizedFleet` is `RandomizedFleet`'s loop around the call with a phase per controller: every member's block carries one more word behind its
bounds, the member's phase as a float (as in an `FR3Fleet`), and the fr3 kernel on the grid (workgroups of N / G rollouts, G, B) reads its controller's word and the
table entry of its (controller, block) pair.  Assignment, phase, state, goal, seed and nominal are a member's own; the plants are shared by all members or a member's
own.  Afterwards each member is bit for bit where its own `update_action()` would have left it, `task.phase` included."""

from __future__ import annotations

from typing import Sequence

import torch

from judo_amd import _lib
from judo_amd.ensemble import MAX_ENSEMBLE
from judo_amd.ensemble_fleet import check_fleet_descriptions, fleet_descriptions
from judo_amd.fr3_ensemble import check_self_collision
from judo_amd.fr3_randomized import FR3RandomizedController, make_fr3_randomized_controller
from judo_amd.optimizers import get_registered_optimizers
from judo_amd.randomized_fleet import RandomizedFleet, fleet_assignments, fleet_weights


class FR3RandomizedFleet(RandomizedFleet):
    """B `FR3RandomizedController`s of one optimizer kind whose plan steps run as one launch.  `fleet[i]` is an ordinary `FR3RandomizedController`: `update_states`,
    `optimizer.seed`, `action(t)`, `traces`, `rewards`, `plant_of_rollout`, `plant_rewards()`, the `assignment` setter, `set_weights`, `set_member` and `task.phase`
    work per member as they do on a controller alone."""

    _fr3_members = True
    _fr3_randomized_members = True
    _block_extra_words = 1  # the phase word, behind the bounds

    def _check_member(self, i: int, c, first) -> None:
        if not isinstance(c, FR3RandomizedController):
            raise ValueError(f"fleet member {i} is a {type(c).__name__}, not an FR3RandomizedController: an FR3RandomizedFleet plans randomised fr3_pick controllers alone "
                             "(judo_amd.fr3_randomized.make_fr3_randomized_controller); every other family's share a launch in a RandomizedFleet")
        if c.task.self_collision != first.task.self_collision or c.model.self_collision != first.model.self_collision:
            raise ValueError(f"fleet member {i} differs from member 0 in self_collision: the launch runs one build of the fr3 kernel")
        super()._check_member(i, c, first)

    def _launch(self, step) -> None:
        """The members' phases (decided by their `pre_rollout` in this iteration) into the phase words, then the B randomised plan steps as one call."""
        self._write_phases(step.fb)
        self._launch_randomized(_lib.lib().jh_plan_step_randomized_batch_phases, step)


def make_fr3_randomized_fleet(optimizer: str, B: int, descriptions: Sequence, blocks: int | None = None, weights=None, self_collision: bool = False,
                              device: torch.device | None = None) -> FR3RandomizedFleet:
    """B `make_fr3_randomized_controller`s in one fleet.  `descriptions`: M model descriptions of fr3_pick, which every member spreads its candidates over, or B lists of
    M, a member's own plants; plant 0 of a list is that member's nominal plant.  `blocks`: the number G of rollout blocks of every member, None: M.  `weights`: M
    non-negative numbers that `blocks_from_weights` turns into every member's assignment, B lists of M for a member's own, or None: block g on plant g % M."""
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
        raise ValueError(f"a set of {M} plants exceeds the {MAX_ENSEMBLE} of a launch (include/judo_amd.h JH_MAX_ENSEMBLE)")
    G = M if blocks is None else int(blocks)
    ws = fleet_weights(B, M, weights)
    fleet_assignments(B, M, G, weights)  # (the limits and the weights, before any device use)
    return FR3RandomizedFleet([make_fr3_randomized_controller(optimizer, lists[i], blocks=G, weights=ws[i], self_collision=self_collision, device=device) for i in range(B)])


__all__ = ["FR3RandomizedFleet", "make_fr3_randomized_fleet"]
