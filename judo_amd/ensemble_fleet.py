"""B ensemble controllers planned in ONE launch (`jh_plan_step_ensemble_batch`, include/judo_amd.h).

An `EnsembleController` plans one nominal against M plants and plans alone: somebody with several robots -- or one robot swept over risk levels (`worst` = 1 ... M),
goals or seeds -- makes B `jh_plan_step_ensemble` calls back to back, B launch chains and B waits for plan steps that each leave most of the GPU idle.  An
`EnsembleFleet` holds B ordinary `EnsembleController` objects and runs their iteration as one call: the rollout kernel on the grid (workgroups, M, B), one aggregating
tail on (tail workgroups, B), one completion mark.  It is `ControllerFleet`'s loop -- every member's host prelude into its slice of the fleet's pinned block, the batched
noise draw, one library call, one `jh_download_end`, every member's epilogue -- around another call, and afterwards each member is bit for bit where its own
`update_action()` would have left it.

What the members share is what the launch shares: `ControllerFleet`'s fields (N, K, H, the spline order, the trace count, the optimizer kind and its scalar arguments),
M, the kernel build, and a model image that differs from fleet member 0's plant 0 in the float section alone.  State, goal, seed, nominal, CEM sigma, `worst` and the
plants themselves are a member's own.  Where all members' plants are byte-identical list for list the launch reads one set of M images; otherwise one of B * M."""

from __future__ import annotations

import ctypes as C
from typing import Sequence

import torch

from judo_amd import _lib
from judo_amd.distributed import world_info
from judo_amd.ensemble import MAX_ENSEMBLE, EnsembleController, check_descriptions, make_ensemble_controller
from judo_amd.fleet import ControllerFleet, _LaunchStep, refuse_fr3_randomized
from judo_amd.models import image_sections
from judo_amd.plants import PlantFleet
from judo_amd.randomized import RandomizedController

MAX_ENSEMBLE_FLEET = _lib.MAX_ENSEMBLE_FLEET


def fleet_descriptions(B: int, descriptions: Sequence) -> list[list[dict]]:
    """`descriptions` as B lists of M: either M descriptions, which every member plans against (the shared form: B times the same list), or B lists of M (the
    per-member form).  Raises ValueError on anything else."""
    if B < 1:
        raise ValueError("a fleet needs at least one controller")
    if B > MAX_ENSEMBLE_FLEET:
        raise ValueError(f"a fleet of {B} ensemble controllers exceeds the {MAX_ENSEMBLE_FLEET} of a launch (include/judo_amd.h JH_MAX_ENSEMBLE_FLEET)")
    descriptions = list(descriptions)
    if not descriptions:
        raise ValueError("an ensemble needs at least one description")
    if all(isinstance(d, dict) for d in descriptions):
        return [list(descriptions) for _ in range(B)]
    if any(isinstance(d, dict) for d in descriptions):
        raise ValueError("descriptions are either M model descriptions, shared by every member, or B lists of M: not a mixture of the two")
    if len(descriptions) != B:
        raise ValueError(f"{len(descriptions)} lists of descriptions for a fleet of {B}")
    return [list(d) for d in descriptions]


def fleet_worst(B: int, M: int, worst) -> list[int]:
    """`worst` as B ints in [1, M]: None is the mean (M for every member), an int holds for every member, a sequence gives one per member."""
    if worst is None:
        out = [M] * B
    elif isinstance(worst, (int,)) and not isinstance(worst, bool):
        out = [int(worst)] * B
    else:
        out = [int(w) for w in worst]
        if len(out) != B:
            raise ValueError(f"{len(out)} values of worst for a fleet of {B}")
    for i, w in enumerate(out):
        if not 1 <= w <= M:
            raise ValueError(f"fleet member {i}: worst = {w} outside [1, M = {M}]")
    return out


def check_fleet_descriptions(lists: Sequence[Sequence[dict]]) -> list[list[bytes]]:
    """The admission rule of an ensemble fleet on descriptions alone, without a device: every member's list is an ensemble (`ensemble.check_descriptions`), all lists
    hold the same number of plants, and every plant's image differs from fleet member 0's plant 0 in the float section alone.  Returns the packed images, list for
    list; raises ValueError naming the member and the field."""
    if len(lists) < 1:
        raise ValueError("a fleet needs at least one controller")
    blobs = []
    for i, descs in enumerate(lists):
        try:
            blobs.append(check_descriptions(descs))
        except ValueError as e:
            raise ValueError(f"fleet member {i}: {e}") from None
    M = len(blobs[0])
    want = image_sections(blobs[0][0])
    for i, mine in enumerate(blobs):
        if len(mine) != M:
            raise ValueError(f"fleet member {i} differs from member 0 in the number of plants M: {len(mine)} against {M}")
        if i == 0 or mine[0] == blobs[0][0]:
            continue  # (the member's other plants were held to its own plant 0 by check_descriptions)
        for name, x, y in zip(("header", "float section", "int section"), image_sections(mine[0]), want):
            if (x != y and name != "float section") or len(x) != len(y):
                raise ValueError(f"fleet member {i} has another model image than member 0: the {name} of its plants' image differs")
    return blobs


class EnsembleFleet(PlantFleet, ControllerFleet):
    """B `EnsembleController`s of one task and optimizer kind whose plan steps run as one launch.  `fleet[i]` is an ordinary `EnsembleController`: `update_states`,
    `optimizer.seed`, `action(t)`, `traces`, `rewards`, `member_costs`, the `worst` setter and `set_member` work per member as they do on a controller alone, and take
    effect at the fleet's next plan step."""

    _ensemble_members = True

    def __init__(self, controllers: Sequence[EnsembleController]) -> None:
        self._member_costs: torch.Tensor | None = None  # (B, M, N): the members' `_member_costs` are views of it
        if len(controllers) > MAX_ENSEMBLE_FLEET:
            raise ValueError(f"a fleet of {len(controllers)} ensemble controllers exceeds the {MAX_ENSEMBLE_FLEET} of a launch (include/judo_amd.h JH_MAX_ENSEMBLE_FLEET)")
        super().__init__(controllers)

    def _check_member(self, i: int, c, first) -> None:
        refuse_fr3_randomized(i, c, self)
        if isinstance(c, RandomizedController):
            raise ValueError(f"fleet member {i} is a RandomizedController: it rolls each candidate out on one plant of its set, not on all of them, and its plan step "
                             "(jh_plan_step_randomized) is another launch; randomised controllers share one in a RandomizedFleet "
                             "(judo_amd.randomized_fleet.make_randomized_fleet)")
        if not isinstance(c, EnsembleController):
            raise ValueError(f"fleet member {i} is a {type(c).__name__}, not an EnsembleController: controllers that believe one plant share a launch in a ControllerFleet")
        world, _ = world_info(c.group)
        why = c._ensemble_refusal(world, c._current_normalizer())
        if why is None and not c.uses_fused_optimizer:
            why = "a plugin reward, hook or optimizer (uses_fused_cost is false): the members' costs come from the fused kernels alone"
        if why is not None:
            raise ValueError(f"fleet member {i} does not run its iteration as one ensemble plan step ({why}): only such controllers can share a launch")
        self._refuse_weights(i, c)
        if c.num_members != first.num_members:
            raise ValueError(f"fleet member {i} differs from member 0 in the number of plants M: {c.num_members} against {first.num_members}")
        self._check_plants(i, c, first)
        super()._check_member(i, c, first)

    @staticmethod
    def _refuse_weights(i: int, c) -> None:
        """A member under the plant-weighted risk measure (`set_weights`) has no place in the launch (`_check_member`: at admission and again in front of every plan step)."""
        if c.weights is not None:
            raise ValueError(f"fleet member {i} has plant weights set (set_weights): the fleet launch carries one `worst` per controller, and B x M weights do not fit in "
                             "its kernel arguments.  set_weights(None) returns the member to the `worst` measure; a weighted controller plans on its own, or shares a launch in a "
                             "WeightedEnsembleFleet (judo_amd.weighted_fleet.make_weighted_ensemble_fleet), whose launch reads a risk record from every member's packed block")

    def _launch(self, step: _LaunchStep) -> None:
        self._launch_ensemble(_lib.lib().jh_plan_step_ensemble_batch, step)

    def _launch_ensemble(self, entry, step: _LaunchStep) -> None:
        """The B ensemble plan steps as one call of `entry`: the set, B, M, the runs, the (B, M, N) member costs the members' `_member_costs` are views of, the costs, `worst`."""
        cs, s = self.controllers, step
        B, M, N = len(cs), cs[0].num_members, s.fb.N
        if self._member_costs is None or tuple(self._member_costs.shape) != (B, M, N):
            self._member_costs = torch.empty((B, M, N), dtype=torch.float32, device=self.device)
        for i, c in enumerate(cs):
            c._member_costs = self._member_costs[i]
        worst = (C.c_int * B)(*[c.worst for c in cs])
        rc = entry(s.model_set.handle, B, M, *s.block, *s.noise_args, *s.sizes, self._member_costs.data_ptr(), s.costs.data_ptr(), worst, *s.update_args, *s.tail)
        _lib.check(rc, entry.__name__)


def make_ensemble_fleet(task: str, optimizer: str, B: int, descriptions: Sequence, worst=None, device: torch.device | None = None) -> EnsembleFleet:
    """B `make_ensemble_controller`s in one fleet.  `descriptions`: M model descriptions of the task, which every member plans against, or B lists of M, a member's own
    plants (`models.scaled_description(task.desc, body_mass=..., geom_friction=..., actuator_kp=...)`); plant 0 of a list is that member's nominal plant.  `worst`: an
    int for every member, a list of B, or None for the mean."""
    lists = fleet_descriptions(B, descriptions)
    check_fleet_descriptions(lists)
    M = len(lists[0])
    if M > MAX_ENSEMBLE:
        raise ValueError(f"an ensemble of {M} members exceeds the {MAX_ENSEMBLE} of a launch (include/judo_amd.h JH_MAX_ENSEMBLE)")
    js = fleet_worst(B, M, worst)
    return EnsembleFleet([make_ensemble_controller(task, optimizer, lists[i], worst=js[i], device=device) for i in range(B)])


__all__ = ["EnsembleFleet", "MAX_ENSEMBLE_FLEET", "check_fleet_descriptions", "fleet_descriptions", "fleet_worst", "make_ensemble_fleet"]
