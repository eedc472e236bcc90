"""The Spot policy tasks on perturbed plants: an ensemble controller and a domain-randomised controller on a `SpotPlantSet` (`jh_policy_rollout_plants`, include/judo_amd.h).

`ensemble.EnsembleController` and `randomized.RandomizedController` are one library call per iteration on a `GpuModelSet`; the Spot policy tasks have neither a `GpuModel`
nor a one-call plan step -- their iteration is spline -> command mapping -> policy + plant rollout -> `Task.reward` -> update.  The two controllers here keep that chain
and give the rollout a plant axis: the tree kernel runs every rollout BLOCK on an image of the set (judo_amd/csrc/jh_engine_v4.hip, PLANTS), the policy step runs on all
rows as before.

  `SpotEnsembleController`    N candidates, each rolled out on all M plants in ONE launch chain of M * N rows; the reward once per member, a risk measure over the M
                              costs (`jh_ensemble_costs`: the mean of the `worst` largest), then the ordinary update.
  `SpotRandomizedController`  N candidates in G blocks of N / G, block g on plant `assignment[g]`: the rollouts of a plain plan step, never fitted to one plant.

Member 0 is the nominal plant: the task's description, `last_rollout` and the traces.  The reference has no counterpart."""

from __future__ import annotations

import warnings
from typing import Sequence

import numpy as np
import torch

from judo_amd import _lib
from judo_amd.config import ControllerConfig
from judo_amd.controller import Controller
from judo_amd.distributed import Shard
from judo_amd.models import layout
from judo_amd.optimizers import get_registered_optimizers
from judo_amd.randomized import blocks_from_weights, check_assignment, plant_of_rollout
from judo_amd.tasks import Task, get_registered_tasks
from judo_amd.tree_model import MAX_TREE_PLANTS, check_tree_descriptions

POLICY_OUTPUT_DIM = 12


class _SpotPlantController(Controller):
    """What the two controllers share: the admission of task and descriptions, the `SpotPlantSet`, `set_member`, the counters, the refusal of the sharded path."""

    _spot_plants = True  # (the fleets refuse such a member: fleet.refuse_fr3_randomized)
    _kind = "plant"  # for messages
    _other_maker = "make_controller"

    def __init__(self, controller_config: ControllerConfig, task: Task, optimizer, descriptions: Sequence[dict], device: torch.device | None = None) -> None:
        if not task.uses_locomotion_policy:
            raise ValueError(f"{type(self).__name__} plans the Spot policy tasks, whose iteration is spline, policy rollout, reward and update; {task.name} does not use the "
                             f"locomotion policy and has a one-call plan step: judo_amd.{self._other_maker} makes its controller")
        check_tree_descriptions(descriptions)
        self._descriptions = list(descriptions)
        task.desc = self._descriptions[0]
        task._layout, task._ctrlrange, task._jadr, task._gpu = layout(task.desc), None, None, None
        super().__init__(controller_config, task, optimizer, device=device)
        from judo_amd.policy import SpotPlantSet

        self.plants = SpotPlantSet(self._descriptions, self.device, self_collision=self.rollout_backend.engine.self_collision)

    @property
    def descriptions(self) -> list[dict]:
        return list(self._descriptions)

    @property
    def num_members(self) -> int:
        return len(self._descriptions)

    def set_member(self, b: int, description: dict) -> None:
        """Replace member b's plant (`SpotPlantSet.set_member`: the library's checks; synchronous -- between plan steps).  b = 0 replaces the nominal plant too."""
        b = int(b)
        if not 0 <= b < len(self._descriptions):
            raise ValueError(f"member {b} of a set of {len(self._descriptions)} plants")
        self.plants.set_member(b, description)
        self._descriptions[b] = description
        if b == 0:
            self.task.desc = description
            self.task._layout, self.task._ctrlrange, self.task._jadr = layout(description), None, None
            self.rollout_backend.engine = self.plants.engines[0]

    def _iteration_shape(self, world: int, nrm) -> str:
        if world > 1 or self.force_shard_path:
            raise ValueError(f"a Spot {self._kind} controller runs its rollouts as one jh_policy_rollout_plants call, which this configuration rules out "
                             f"(a process group or force_shard_path: the sharded path has no {self._kind} form)")
        return super()._iteration_shape(world, nrm)

    def _candidates_iteration(self, lib, b, nrm, nominal_n, W, shard: Shard, H, K, nu, N, stream, state):
        if shard.world > 1:
            raise ValueError(f"a Spot {self._kind} controller runs its rollouts as one jh_policy_rollout_plants call, which this configuration rules out "
                             f"(a process group or force_shard_path: the sharded path has no {self._kind} form)")
        return super()._candidates_iteration(lib, b, nrm, nominal_n, W, shard, H, K, nu, N, stream, state)

    def solver_stats(self, reset: bool = True) -> dict:
        """`Controller.solver_stats` from the set's counters: the plan steps' launches run on the set, not on a member's engine."""
        st = self.plants.stats(reset)
        st = {"contact_overflow": st["contacts_dropped"], "newton_cap_hits": st["steps_at_cap"], "newton_iters": st["newton_iterations"], "steps": st["steps"]}
        if self.solver_warnings and st["steps"] > 0 and (st["contact_overflow"] > 1e-4 * st["steps"] or st["newton_cap_hits"] > 1e-2 * st["steps"]):
            warnings.warn(f"{self.task.name}: {st['contact_overflow']} contacts dropped above the kernel's per-rollout capacity and {st['newton_cap_hits']} "
                          f"constraint solves stopped at the iteration cap in {st['steps']} physics steps -- those rollouts are approximate", stacklevel=2)
        return st

    def _spline_commands(self, nom_d, noise_p, ldn: int, sig_d, lohi_d, knots_nku, W, shard: Shard, H: int, K: int, stream) -> tuple[torch.Tensor, torch.Tensor]:
        """The candidates' controls at the rollout times (`jh_spline_controls`, once) and the policy commands they map to."""
        lib, nu = _lib.lib(), self.nu
        controls = torch.empty((shard.count, H, nu), dtype=torch.float32, device=self.device)
        st = lib.jh_spline_controls(_lib.ptr(W), _lib.ptr(knots_nku), _lib.ptr(nom_d), noise_p, ldn, _lib.ptr(sig_d), _lib.ptr(lohi_d) if knots_nku is None else None,
                                    shard.count, shard.offset, H, K, nu, _lib.ptr(controls), stream)
        _lib.check(st, "jh_spline_controls")
        return controls, self.task.task_to_sim_ctrl(controls).to(torch.float32).contiguous()


class SpotEnsembleController(_SpotPlantController):
    """A Spot `Controller` whose iteration rolls every candidate out on M plants and updates on the aggregated costs.  `rewards` are the negated aggregated costs;
    `member_costs` / `member_rewards` the (M, N) costs behind them; `worst` may be set between plan steps, and `set_member(b, description)` replaces one plant.
    The carried state is the (M * N, 12) policy outputs and the (M * N, nv) warm start of the plant rollout, reset wherever the controller resets its own."""

    _kind = "ensemble"
    _other_maker = "ensemble.make_ensemble_controller"

    def __init__(self, controller_config: ControllerConfig, task: Task, optimizer, descriptions: Sequence[dict], worst: int | None = None,
                 device: torch.device | None = None) -> None:
        self._plant_backend = None
        self._plant_policy_out: torch.Tensor | None = None
        self._member_costs: torch.Tensor | None = None
        M = len(descriptions)
        if worst is not None and not 1 <= int(worst) <= M:
            raise ValueError(f"worst = {worst} outside [1, M = {M}]")
        self._worst = M if worst is None else int(worst)
        super().__init__(controller_config, task, optimizer, descriptions, device=device)

    @property
    def worst(self) -> int:
        """How many of a rollout's largest member costs are averaged: 1 = the worst case, M = the mean."""
        return self._worst

    @worst.setter
    def worst(self, j: int) -> None:
        if not 1 <= int(j) <= len(self._descriptions):
            raise ValueError(f"worst = {j} outside [1, M = {len(self._descriptions)}]")
        self._worst = int(j)

    @property
    def member_costs(self) -> np.ndarray:
        """(M, N) fp32: member m's cost of every candidate of the last iteration."""
        if self._member_costs is None:
            raise RuntimeError("member_costs needs a completed update_action()")
        return self._member_costs.cpu().numpy()

    @property
    def member_rewards(self) -> np.ndarray:
        return -self.member_costs.astype(np.float64)

    def reset(self) -> None:
        super().reset()
        self._plant_policy_out = None  # re-created as zeros by the next rollout, with the plant backend's warm start
        if self._plant_backend is not None:
            self._plant_backend.update(self._plant_backend.num_threads)

    def _carried(self, rows: int):
        """The backend of M * N threads around the controller's engine and policy, and the (M * N, 12) policy outputs; both start from zero when the row count changes
        (a live change of `num_rollouts`), as the controller's own do."""
        from judo_amd.policy import PolicyRolloutBackend

        own = self.rollout_backend
        pb = self._plant_backend
        if pb is None or pb.policy is not own.policy:
            pb = self._plant_backend = PolicyRolloutBackend(rows, physics_substeps=own.physics_substeps, device=self.device, carry_warmstart=own.carry_warmstart, share=own)
            self._plant_policy_out = None
        if pb.num_threads != rows:
            pb.update(rows)
            self._plant_policy_out = None
        if self._plant_policy_out is None or self._last_policy_output is None:  # (`_begin_plan` drops the controller's own outputs when the rollouts change)
            self._plant_policy_out = torch.zeros((rows, POLICY_OUTPUT_DIM), dtype=torch.float32, device=self.device)
            pb.update(rows)
            self._last_policy_output = self._plant_policy_out[: rows // len(self._descriptions)]
        return pb, self._plant_policy_out

    def _materialised_costs(self, x0_d, nom_d, noise_p, ldn: int, sig_d, lohi_d, knots_nku, W, shard: Shard, H: int, K: int, stream) -> torch.Tensor:
        lib = _lib.lib()
        M, N = len(self._descriptions), shard.count
        controls, commands = self._spline_commands(nom_d, noise_p, ldn, sig_d, lohi_d, knots_nku, W, shard, H, K, stream)
        pb, policy_out = self._carried(M * N)
        nx = self.plants.nq + self.plants.nv
        states, sensors = pb.rollout_plants(self.plants, x0_d, nx, 1, M, list(range(M)), commands.repeat(M, 1, 1), policy_out, cutoff_time=self.rollout_cutoff_time)
        if self._member_costs is None or tuple(self._member_costs.shape) != (M, N):
            self._member_costs = torch.empty((M, N), dtype=torch.float32, device=self.device)
        for m in range(M):  # the reward per member, in the shapes a plain controller gives it
            self._score_rollout(states[m * N : (m + 1) * N], sensors[m * N : (m + 1) * N], controls, out=self._member_costs[m])
        self.last_rollout = (states[:N], sensors[:N], controls)  # member 0, the nominal plant
        costs = torch.empty(N, dtype=torch.float32, device=self.device)
        _lib.check(lib.jh_ensemble_costs(_lib.ptr(self._member_costs), M, N, N, self._worst, _lib.ptr(costs), stream), "jh_ensemble_costs")
        return costs


class SpotRandomizedController(_SpotPlantController):
    """A Spot `Controller` whose iteration rolls block g of its candidates out on plant `assignment[g]` and updates on the N costs as they are.  `assignment` (G plant
    indices, default g % M) may be set between plan steps -- it travels in the kernel arguments; `plant_of_rollout` and `plant_rewards()` say which plant a reward
    belongs to, and `set_member(b, description)` replaces one plant.  The carried policy outputs and warm start are the controller's own N rows."""

    _kind = "randomised"
    _other_maker = "randomized.make_randomized_controller"

    def __init__(self, controller_config: ControllerConfig, task: Task, optimizer, descriptions: Sequence[dict], blocks: int | None = None,
                 weights: Sequence[float] | None = None, device: torch.device | None = None) -> None:
        M = len(descriptions)
        G = M if blocks is None else int(blocks)
        if weights is not None and len(weights) != M:
            raise ValueError(f"{len(weights)} weights for M = {M} plants")
        self._assignment = check_assignment(blocks_from_weights(weights, G) if weights is not None else [g % max(M, 1) for g in range(max(G, 0))], M)
        self._assignment_used: list[int] | None = None  # the assignment of the last plan step: what `rewards` were rolled out on
        super().__init__(controller_config, task, optimizer, descriptions, device=device)

    @property
    def blocks(self) -> int:
        return len(self._assignment)

    @property
    def assignment(self) -> list[int]:
        """The plant of every rollout block, G indices in [0, M), validated when set.  Setting it takes effect at the next plan step and costs nothing on the device;
        `update_action` raises ValueError if the G blocks do not divide `num_rollouts` then."""
        return list(self._assignment)

    @assignment.setter
    def assignment(self, a: Sequence[int]) -> None:
        self._assignment = check_assignment(a, len(self._descriptions))

    def set_weights(self, weights: Sequence[float], blocks: int | None = None) -> None:
        """`assignment = blocks_from_weights(weights, blocks)`; `blocks` None keeps the number of blocks."""
        if len(weights) != len(self._descriptions):
            raise ValueError(f"{len(weights)} weights for M = {len(self._descriptions)} plants")
        self.assignment = blocks_from_weights(weights, len(self._assignment) if blocks is None else blocks)

    @property
    def plant_of_rollout(self) -> np.ndarray:
        """(N,) ints: the plant every rollout of the last plan step ran on (of the next one, before the first)."""
        if self._assignment_used is None:
            return plant_of_rollout(self._assignment, self.optimizer.num_rollouts)
        return plant_of_rollout(self._assignment_used, int(self.costs_device.numel()))

    def plant_rewards(self) -> np.ndarray:
        """(M,) fp64: the mean of `rewards` over the rollouts of every plant, NaN for a plant with no block."""
        r, plant = np.asarray(self.rewards, dtype=np.float64), self.plant_of_rollout
        return np.array([r[plant == m].mean() if (plant == m).any() else np.nan for m in range(len(self._descriptions))])

    def update_action(self) -> None:
        if self.optimizer_cfg.num_rollouts > 0 and self.optimizer_cfg.num_rollouts % len(self._assignment) != 0:  # (a live change of num_rollouts)
            raise ValueError(f"num_rollouts % blocks != 0: {self.optimizer_cfg.num_rollouts} rollouts do not split into {len(self._assignment)} equal blocks")
        super().update_action()

    def _materialised_costs(self, x0_d, nom_d, noise_p, ldn: int, sig_d, lohi_d, knots_nku, W, shard: Shard, H: int, K: int, stream) -> torch.Tensor:
        N, a = shard.count, list(self._assignment)
        controls, commands = self._spline_commands(nom_d, noise_p, ldn, sig_d, lohi_d, knots_nku, W, shard, H, K, stream)
        if self._last_policy_output is None:
            self._last_policy_output = torch.zeros((N, POLICY_OUTPUT_DIM), dtype=torch.float32, device=self.device)
        nx = self.plants.nq + self.plants.nv
        states, sensors = self.rollout_backend.rollout_plants(self.plants, x0_d, nx, 1, len(a), a, commands, self._last_policy_output, cutoff_time=self.rollout_cutoff_time)
        self._assignment_used = a
        return self._score_rollout(states, sensors, controls)


def _make(cls, task: str | Task, optimizer: str, descriptions: Sequence[dict], device, **kw):
    tasks, opts = get_registered_tasks(), get_registered_optimizers()
    if isinstance(task, str):
        if task not in tasks:
            raise ValueError(f"Task {task} not found in task registry.")
        task = tasks[task][0]()
    if optimizer not in opts:
        raise ValueError(f"Optimizer {optimizer} not found in optimizer registry.")
    opt_cls, opt_cfg_cls = opts[optimizer]
    opt_cfg = opt_cfg_cls()
    opt_cfg.set_override(task.name)
    ctrl_cfg = ControllerConfig()
    ctrl_cfg.set_override(task.name)
    return cls(ctrl_cfg, task, opt_cls(opt_cfg, task.nu), descriptions, device=device, **kw)


def make_spot_ensemble_controller(task: str | Task, optimizer: str, descriptions: Sequence[dict], worst: int | None = None,
                                  device: torch.device | None = None) -> SpotEnsembleController:
    """`make_controller` for one Spot controller over M plants: the registered task and optimizer (with the task's overrides) around `descriptions`, M descriptions of the
    task's model (`models.scaled_description(task.desc, body_mass=..., geom_friction=..., actuator_kp=...)`).  Member 0 is the nominal plant.  `worst`: how many of a
    candidate's largest member costs are averaged; None: all M, the mean."""
    return _make(SpotEnsembleController, task, optimizer, descriptions, device, worst=worst)


def make_spot_randomized_controller(task: str | Task, optimizer: str, descriptions: Sequence[dict], blocks: int | None = None, weights: Sequence[float] | None = None,
                                    device: torch.device | None = None) -> SpotRandomizedController:
    """`make_controller` for one Spot controller whose candidates are spread over M plants.  `blocks`: the number G of rollout blocks, None: M; `weights`: M non-negative
    numbers that `randomized.blocks_from_weights` turns into the assignment, None: block g on plant g % M.  G must divide `num_rollouts` at the plan step."""
    return _make(SpotRandomizedController, task, optimizer, descriptions, device, blocks=blocks, weights=weights)


__all__ = ["MAX_TREE_PLANTS", "SpotEnsembleController", "SpotRandomizedController", "check_tree_descriptions", "make_spot_ensemble_controller",
           "make_spot_randomized_controller"]
