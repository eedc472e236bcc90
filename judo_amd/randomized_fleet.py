"""B domain-randomised controllers planned in ONE launch (`jh_plan_step_randomized_batch`, include/judo_amd.h).

A `RandomizedController` spreads the N candidates of one plan step over the M plants of its set, block by block, and pays what a plain plan step pays -- which is why it
is the one somebody runs at shipped sizes, and why B of them back to back, B launch chains and B waits, leave most of the GPU idle.  A `RandomizedFleet` holds B
ordinary `RandomizedController` objects and runs their iteration as one call: the rollout kernel on the grid (workgroups of N / G rollouts, G, B), every controller with
its own table from block to plant, then the batched tail on (tail workgroups, B) and one completion mark.  It is `ControllerFleet`'s loop around another call, and
afterwards each member is bit for bit where its own `update_action()` would have left it.

What the members share is what the launch shares: `ControllerFleet`'s fields (N, K, H, the spline order, the trace count, the optimizer kind and its scalar arguments),
M, the number of blocks G (a grid dimension), the kernel build, and a model image that differs from fleet member 0's plant 0 in the float section alone.  State, goal,
seed, nominal, CEM sigma, the assignment and the plants themselves are a member's own.  Where all members' plants are byte-identical list for list the launch reads one
set of M images; otherwise one of B * M.  The B assignments travel in the kernel arguments, B * G bytes: another draw for the next plan step costs no copy."""

from __future__ import annotations

import ctypes as C
from typing import Sequence

import torch

from judo_amd import _lib
from judo_amd.distributed import world_info
from judo_amd.ensemble import MAX_ENSEMBLE
from judo_amd.ensemble_fleet import MAX_ENSEMBLE_FLEET, check_fleet_descriptions, fleet_descriptions
from judo_amd.fleet import ControllerFleet, _LaunchStep, refuse_fr3_randomized
from judo_amd.plants import PlantFleet
from judo_amd.randomized import MAX_PLANT_BLOCKS, RandomizedController, blocks_from_weights, check_task, make_randomized_controller
from judo_amd.tasks import get_registered_tasks

MAX_FLEET_PLANT_BLOCKS = _lib.MAX_FLEET_PLANT_BLOCKS


def check_fleet_blocks(B: int, G: int) -> None:
    """The launch's limits on B controllers of G blocks each; raises ValueError naming the one that is exceeded."""
    if B < 1:
        raise ValueError("a fleet needs at least one controller")
    if B > MAX_ENSEMBLE_FLEET:
        raise ValueError(f"a fleet of {B} randomised controllers exceeds the {MAX_ENSEMBLE_FLEET} of a launch (include/judo_amd.h JH_MAX_ENSEMBLE_FLEET)")
    if not 1 <= G <= MAX_PLANT_BLOCKS:
        raise ValueError(f"{G} blocks are outside [1, {MAX_PLANT_BLOCKS}] (include/judo_amd.h JH_MAX_PLANT_BLOCKS)")
    if B * G > MAX_FLEET_PLANT_BLOCKS:
        raise ValueError(f"B * G = {B} * {G} = {B * G} (controller, block) pairs exceed the {MAX_FLEET_PLANT_BLOCKS} of a launch (include/judo_amd.h JH_MAX_FLEET_PLANT_BLOCKS)")


def fleet_weights(B: int, M: int, weights) -> list[list[float] | None]:
    """`weights` as B lists of M numbers (or B times None): None is every member's default assignment, M numbers hold for every member, B lists of M give a member's
    own.  Raises ValueError on anything else."""
    if weights is None:
        return [None] * B
    weights = list(weights)
    nested = [hasattr(w, "__len__") for w in weights]
    if not any(nested):
        if len(weights) != M:
            raise ValueError(f"{len(weights)} weights for M = {M} plants")
        return [[float(w) for w in weights] for _ in range(B)]
    if not all(nested):
        raise ValueError("weights are either M numbers, shared by every member, or B lists of M: not a mixture of the two")
    if len(weights) != B:
        raise ValueError(f"{len(weights)} lists of weights for a fleet of {B}")
    out = []
    for i, w in enumerate(weights):
        if len(w) != M:
            raise ValueError(f"fleet member {i}: {len(w)} weights for M = {M} plants")
        out.append([float(x) for x in w])
    return out


def fleet_assignments(B: int, M: int, G: int, weights) -> list[list[int]]:
    """The B assignments a `make_randomized_fleet` call starts from, without a device: `blocks_from_weights` per member (largest remainder), or block g on plant
    g % M where there are no weights."""
    check_fleet_blocks(B, G)
    out = []
    for i, w in enumerate(fleet_weights(B, M, weights)):
        try:
            out.append([g % M for g in range(G)] if w is None else blocks_from_weights(w, G))
        except ValueError as e:
            raise ValueError(f"fleet member {i}: {e}") from None
    return out


class RandomizedFleet(PlantFleet, ControllerFleet):
    """B `RandomizedController`s of one task and optimizer kind whose plan steps run as one launch.  `fleet[i]` is an ordinary `RandomizedController`: `update_states`,
    `optimizer.seed`, `action(t)`, `traces`, `rewards`, `plant_of_rollout`, `plant_rewards()`, the `assignment` setter, `set_weights` and `set_member` work per member as
    they do on a controller alone, and take effect at the fleet's next plan step."""

    _randomized_members = True

    def __init__(self, controllers: Sequence[RandomizedController]) -> None:
        if len(controllers) > MAX_ENSEMBLE_FLEET:
            raise ValueError(f"a fleet of {len(controllers)} randomised controllers exceeds the {MAX_ENSEMBLE_FLEET} of a launch (include/judo_amd.h JH_MAX_ENSEMBLE_FLEET)")
        super().__init__(controllers)

    def _check_member(self, i: int, c, first) -> None:
        refuse_fr3_randomized(i, c, self)
        if not isinstance(c, RandomizedController):
            raise ValueError(f"fleet member {i} is a {type(c).__name__}, not a RandomizedController: controllers that believe one plant share a launch in a ControllerFleet, "
                             "ensemble controllers in an EnsembleFleet")
        world, _ = world_info(c.group)
        why = c._randomized_refusal(world, c._current_normalizer())
        if why is None and not c.uses_fused_optimizer:
            why = "a plugin reward, hook or optimizer (uses_fused_cost is false): the plants' costs come from the fused kernels alone"
        if why is not None:
            raise ValueError(f"fleet member {i} does not run its iteration as one jh_plan_step_randomized call ({why}): only such controllers can share a launch")
        if c.num_members != first.num_members:
            raise ValueError(f"fleet member {i} differs from member 0 in the number of plants M: {c.num_members} against {first.num_members}")
        if c.blocks != first.blocks:
            raise ValueError(f"fleet member {i} differs from member 0 in the number of blocks G: {c.blocks} against {first.blocks} (G is a grid dimension of the launch)")
        if i == 0:
            check_fleet_blocks(len(self.controllers), c.blocks)
        self._check_plants(i, c, first)
        super()._check_member(i, c, first)

    def update_action(self) -> None:
        first = self.controllers[0]
        N, G = first.optimizer_cfg.num_rollouts, first.blocks
        if N > 0 and N % G != 0:  # (a live change of num_rollouts; the members agree in both, _check_member)
            raise ValueError(f"num_rollouts % blocks != 0: {N} rollouts do not split into {G} equal blocks")
        super().update_action()

    def _launch(self, step: _LaunchStep) -> None:
        self._launch_randomized(_lib.lib().jh_plan_step_randomized_batch, step)

    def _launch_randomized(self, entry, step: _LaunchStep) -> None:
        """The B randomised plan steps as one call of `entry`: the set, B, M, the runs, the B assignments in force (which become the members' `_assignment_used`), G, the costs."""
        cs, s = self.controllers, step
        B, M, G = len(cs), cs[0].num_members, cs[0].blocks
        used = [list(c._assignment) for c in cs]  # the B assignments in force, controller-major
        table = (C.c_ubyte * (B * G))(*[p for a in used for p in a])
        rc = entry(s.model_set.handle, B, M, *s.block, *s.noise_args, *s.sizes, table, G, s.costs.data_ptr(), *s.update_args, *s.tail)
        _lib.check(rc, entry.__name__)
        for c, a in zip(cs, used):
            c._assignment_used = a


def make_randomized_fleet(task: str, optimizer: str, B: int, descriptions: Sequence, blocks: int | None = None, weights=None,
                          device: torch.device | None = None) -> RandomizedFleet:
    """B `make_randomized_controller`s in one fleet.  `descriptions`: M model descriptions of the task, which every member spreads its candidates over, or B lists of M,
    a member's own plants (`models.scaled_description(task.desc, body_mass=..., geom_friction=..., actuator_kp=...)`); plant 0 of a list is that member's nominal
    plant.  `blocks`: the number G of rollout blocks of every member, None: M.  `weights`: M non-negative numbers that `blocks_from_weights` turns into every member's
    assignment, B lists of M for a member's own, or None: block g on plant g % M."""
    tasks = get_registered_tasks()
    if task not in tasks:
        raise ValueError(f"Task {task} not found in task registry.")
    check_task(tasks[task][0]())  # (fr3_pick and the Spot policy tasks, with the single controller's messages, before anything is packed)
    lists = fleet_descriptions(B, descriptions)
    check_fleet_descriptions(lists)
    M = len(lists[0])
    if M > MAX_ENSEMBLE:
        raise ValueError(f"a set of {M} plants exceeds the {MAX_ENSEMBLE} of a launch (include/judo_amd.h JH_MAX_ENSEMBLE)")
    G = M if blocks is None else int(blocks)
    ws = fleet_weights(B, M, weights)
    fleet_assignments(B, M, G, weights)  # (the limits and the weights, before any device use)
    return RandomizedFleet([make_randomized_controller(task, optimizer, lists[i], blocks=G, weights=ws[i], device=device) for i in range(B)])


__all__ = ["MAX_FLEET_PLANT_BLOCKS", "RandomizedFleet", "check_fleet_blocks", "fleet_assignments", "fleet_weights", "make_randomized_fleet"]
