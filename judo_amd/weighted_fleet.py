"""B ensemble controllers planned in ONE launch, each under a risk measure of its own (`jh_plan_step_ensemble_batch_risk`, include/judo_amd.h).

A `PlantEstimator` turns a robot's observed steps into a posterior over the plants of its model set, and `apply_risk` hands that posterior to an ensemble controller
as the weights of a tail mean (`set_weights`).  An `EnsembleFleet` refuses such a member: its launch carries one `worst` per controller in the kernel arguments, and
B x M weights -- up to 32 KB -- do not fit there.  So B robots that have each learned something about their own plant were back to B launch chains and B waits.

A `WeightedEnsembleFleet` is `EnsembleFleet`'s loop around the call that reads the measure from memory: every member's block carries 1 + M more words behind its
bounds, the member's risk record -- the tail word, 0.0 for the `worst` measure, then the M weights --, as an fr3 fleet's blocks carry the phase word.  The record
rides on the block upload that happens anyway (or is read in place where the kernel reads the pinned host block), and the batched tail reads it as wave-uniform loads:
following B beliefs costs no copy and no launch.  Members may be weighted, unweighted or mixed, and may change between plan steps through `set_weights`,
`set_weights(None)`, the `worst` setter and `PlantEstimator.apply_risk(fleet[i], ...)`.  Afterwards each member is bit for bit where its own `update_action()` would have
left it.  An `FR3WeightedEnsembleFleet` is the same for fr3_pick: the phase word first, the risk record behind it."""

from __future__ import annotations

from typing import Sequence

import numpy as np
import torch

from judo_amd import _lib
from judo_amd.ensemble import MAX_ENSEMBLE, make_ensemble_controller
from judo_amd.ensemble_fleet import EnsembleFleet, check_fleet_descriptions, fleet_descriptions, fleet_worst
from judo_amd.fr3_ensemble import FR3EnsembleFleet, check_self_collision, make_fr3_ensemble_controller
from judo_amd.optimizers import get_registered_optimizers
from judo_amd.randomized_fleet import fleet_weights
from judo_amd.tasks import get_registered_tasks


def risk_record(c) -> np.ndarray:
    """Member `c`'s risk record, (1 + M,) fp32: [0.0, 0 ...] under the `worst` measure (the launch takes `worst` itself from the kernel arguments), else
    [tail, weights]."""
    w = c.weights
    rec = np.zeros(1 + c.num_members, dtype=np.float32)
    if w is not None:
        rec[0], rec[1:] = c.tail, w
    return rec


def fleet_tails(B: int, tail) -> list[float | None]:
    """`tail` as B values: None keeps every member's own (`worst / M`), a number holds for every member, a sequence gives one per member.  Each lies in (0, 1]."""
    if tail is None:
        return [None] * B
    out = [float(t) for t in tail] if hasattr(tail, "__len__") else [float(tail)] * B
    if len(out) != B:
        raise ValueError(f"{len(out)} values of tail for a fleet of {B}")
    for i, t in enumerate(out):
        if not 0 < float(np.float32(t)) <= 1:  # (false for NaN)
            raise ValueError(f"fleet member {i}: tail = {t} outside (0, 1]")
    return out


class _RiskRecords:
    """What both weighted fleets add to their ensemble fleet: the members' risk records in the fleet's words of their blocks, and the entry that reads them."""

    _risk_at = 0  # where in a block's fleet words the risk record begins (behind the phase word, where the blocks have one)

    @staticmethod
    def _refuse_weights(i: int, c) -> None:
        """Weighted members are what this fleet is for: nothing is refused (`set_weights` validated the weights and the tail when they were set)."""

    @property
    def _block_extra_words(self) -> int:
        return self._risk_at + 1 + self.controllers[0].num_members

    @property
    def _block_extra_at(self) -> tuple:
        return tuple(range(self._risk_at + 1))  # (the phase word, if any, then the risk record: the offsets the entry takes behind o_lohi)

    def _write_risk(self, fb) -> None:
        """The members' risk records, as they stand in front of this launch, into the fleet's words of their host blocks."""
        for i, c in enumerate(self.controllers):
            at = i * fb.blk_stride + fb.nblk + self._risk_at
            fb.host_np[at : at + 1 + c.num_members] = risk_record(c)


class WeightedEnsembleFleet(_RiskRecords, EnsembleFleet):
    """B `EnsembleController`s of one task and optimizer kind whose plan steps run as one launch, each under its own risk measure: `fleet[i].set_weights(p, tail)`,
    `set_weights(None)`, the `worst` setter and `PlantEstimator.apply_risk(fleet[i], ...)` take effect at the fleet's next plan step.  Every admission rule but the
    refusal of weights is `EnsembleFleet`'s."""

    def _launch(self, step) -> None:
        self._write_risk(step.fb)
        self._launch_ensemble(_lib.lib().jh_plan_step_ensemble_batch_risk, step)


class FR3WeightedEnsembleFleet(_RiskRecords, FR3EnsembleFleet):
    """`WeightedEnsembleFleet` for fr3_pick: B `FR3EnsembleController`s, a phase and a risk measure per member."""

    _risk_at = 1  # (the phase word stays the first of the fleet's words: o_phase is what it is in an FR3EnsembleFleet)

    def _launch(self, step) -> None:
        self._write_phases(step.fb)
        self._write_risk(step.fb)
        self._launch_ensemble(_lib.lib().jh_plan_step_ensemble_batch_phases_risk, step)


def _fleet_risk(B: int, lists: Sequence[Sequence[dict]], worst, weights, tail) -> tuple[list[int], list, list]:
    """The makers' checks behind the descriptions', without a device: M, `worst`, the weights and the tails of the B members."""
    M = len(lists[0])
    if M > MAX_ENSEMBLE:
        raise ValueError(f"an ensemble of {M} members exceeds the {MAX_ENSEMBLE} of a launch (include/judo_amd.h JH_MAX_ENSEMBLE)")
    ws, ts = fleet_weights(B, M, weights), fleet_tails(B, tail)
    for i, w in enumerate(ws):
        if w is not None and (not np.isfinite(w).all() or min(w) < 0 or not sum(w) > 0):
            raise ValueError(f"fleet member {i}: weights must be non-negative, finite numbers with a positive sum, got {w}")
    return fleet_worst(B, M, worst), ws, ts


def _with_risk(c, weights, tail):
    if weights is not None or tail is not None:
        c.set_weights(weights, tail)
    return c


def make_weighted_ensemble_fleet(task: str, optimizer: str, B: int, descriptions: Sequence, worst=None, weights=None, tail=None,
                                 device: torch.device | None = None) -> WeightedEnsembleFleet:
    """B `make_ensemble_controller`s in one `WeightedEnsembleFleet`.  `descriptions` and `worst` as for `make_ensemble_fleet`.  `weights`: M numbers for every member, B
    lists of M for a member's own, or None: every member starts under its `worst` measure.  `tail`: a float for every member or B floats, in (0, 1]; None: a member's
    own `worst / M`.  A tail without weights is kept for the weights a member gets later."""
    tasks = get_registered_tasks()
    if task not in tasks:
        raise ValueError(f"Task {task} not found in task registry.")
    lists = fleet_descriptions(B, descriptions)
    check_fleet_descriptions(lists)
    js, ws, ts = _fleet_risk(B, lists, worst, weights, tail)
    return WeightedEnsembleFleet([_with_risk(make_ensemble_controller(task, optimizer, lists[i], worst=js[i], device=device), ws[i], ts[i]) for i in range(B)])


def make_fr3_weighted_ensemble_fleet(optimizer: str, B: int, descriptions: Sequence, worst=None, weights=None, tail=None, self_collision: bool = False,
                                     device: torch.device | None = None) -> FR3WeightedEnsembleFleet:
    """B `make_fr3_ensemble_controller`s in one `FR3WeightedEnsembleFleet`: `make_fr3_ensemble_fleet`'s arguments with `weights` and `tail` as above."""
    if optimizer not in get_registered_optimizers():
        raise ValueError(f"Optimizer {optimizer} not found in optimizer registry.")
    lists = fleet_descriptions(B, descriptions)
    for i, descs in enumerate(lists):
        try:
            check_self_collision(descs, self_collision)
        except ValueError as e:
            raise ValueError(f"fleet member {i}: {e}") from None
    check_fleet_descriptions(lists)
    js, ws, ts = _fleet_risk(B, lists, worst, weights, tail)
    return FR3WeightedEnsembleFleet(
        [_with_risk(make_fr3_ensemble_controller(optimizer, lists[i], worst=js[i], self_collision=self_collision, device=device), ws[i], ts[i]) for i in range(B)])


__all__ = ["FR3WeightedEnsembleFleet", "WeightedEnsembleFleet", "fleet_tails", "make_fr3_weighted_ensemble_fleet", "make_weighted_ensemble_fleet", "risk_record"]
