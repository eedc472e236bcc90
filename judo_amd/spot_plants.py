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

import torch

from judo_amd.config import ControllerConfig
from judo_amd.controller import Controller
from judo_amd.plants import Assignment, PlantSet, WorstCase, make_for, spline_controls
from judo_amd.tasks import Task
from judo_amd.tree_model import MAX_TREE_PLANTS, check_tree_descriptions

POLICY_OUTPUT_DIM = 12


class _SpotPlantController(PlantSet, Controller):
    """What the two controllers share: the admission of task and descriptions, the `SpotPlantSet` behind `plants.PlantSet`'s `set_member`, the counters, the refusal of
    the sharded path."""

    _spot_plants = True  # (the fleets refuse such a member: fleet.refuse_fr3_randomized)
    _kind = "plant"  # for messages
    _other_maker = "make_controller"

    def __init__(self, controller_config: ControllerConfig, task: Task, optimizer, descriptions: Sequence[dict], device: torch.device | None = None) -> None:
        if not task.uses_locomotion_policy:
            raise ValueError(f"{type(self).__name__} plans the Spot policy tasks, whose iteration is spline, policy rollout, reward and update; {task.name} does not use the "
                             f"locomotion policy and has a one-call plan step: judo_amd.{self._other_maker} makes its controller")
        check_tree_descriptions(descriptions)
        self._descriptions = list(descriptions)
        super().__init__(controller_config, task, optimizer, device=device)

    def _make_set(self) -> None:
        from judo_amd.policy import SpotPlantSet

        self.plants = SpotPlantSet(self._descriptions, self.device, self_collision=self.rollout_backend.engine.self_collision)

    def _replace_plant(self, b: int, description: dict) -> None:
        """`SpotPlantSet.set_member`: the library's checks."""
        self.plants.set_member(b, description)
        if b == 0:
            self.rollout_backend.engine = self.plants.engines[0]

    def _iteration_shape(self, world: int, nrm) -> str:
        if world > 1 or self.force_shard_path:
            raise ValueError(f"a Spot {self._kind} controller runs its rollouts as one jh_policy_rollout_plants call, which this configuration rules out "
                             f"(a process group or force_shard_path: the sharded path has no {self._kind} form)")
        return super()._iteration_shape(world, nrm)

    def _candidates_iteration(self, plan, b, st) -> None:
        if plan.shard.world > 1:
            raise ValueError(f"a Spot {self._kind} controller runs its rollouts as one jh_policy_rollout_plants call, which this configuration rules out "
                             f"(a process group or force_shard_path: the sharded path has no {self._kind} form)")
        super()._candidates_iteration(plan, b, st)

    def solver_stats(self, reset: bool = True) -> dict:
        """`Controller.solver_stats` from the set's counters: the plan steps' launches run on the set, not on a member's engine."""
        st = self.plants.stats(reset)
        st = {"contact_overflow": st["contacts_dropped"], "newton_cap_hits": st["steps_at_cap"], "newton_iters": st["newton_iterations"], "steps": st["steps"]}
        if self.solver_warnings and st["steps"] > 0 and (st["contact_overflow"] > 1e-4 * st["steps"] or st["newton_cap_hits"] > 1e-2 * st["steps"]):
            warnings.warn(f"{self.task.name}: {st['contact_overflow']} contacts dropped above the kernel's per-rollout capacity and {st['newton_cap_hits']} "
                          f"constraint solves stopped at the iteration cap in {st['steps']} physics steps -- those rollouts are approximate", stacklevel=2)
        return st

    def _spline_commands(self, plan, b, st) -> tuple[torch.Tensor, torch.Tensor]:
        """The candidates' controls at the rollout times (`plants.spline_controls`, once) and the policy commands they map to."""
        controls = spline_controls(self, plan, b, st)
        return controls, self.task.task_to_sim_ctrl(controls).to(torch.float32).contiguous()


class SpotEnsembleController(WorstCase, _SpotPlantController):
    """A Spot `Controller` whose iteration rolls every candidate out on M plants and updates on the aggregated costs.  `rewards` are the negated aggregated costs;
    `member_costs` / `member_rewards` the (M, N) costs behind them; `worst` may be set between plan steps, and `set_member(b, description)` replaces one plant.
    The carried state is the (M * N, 12) policy outputs and the (M * N, nv) warm start of the plant rollout, reset wherever the controller resets its own."""

    _kind = "ensemble"
    _other_maker = "ensemble.make_ensemble_controller"

    def __init__(self, controller_config: ControllerConfig, task: Task, optimizer, descriptions: Sequence[dict], worst: int | None = None,
                 device: torch.device | None = None) -> None:
        self._plant_backend = None
        self._plant_policy_out: torch.Tensor | None = None
        self._init_worst(worst, len(descriptions))
        super().__init__(controller_config, task, optimizer, descriptions, device=device)

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

    def _materialised_costs(self, plan, b, st) -> torch.Tensor:
        M, N = len(self._descriptions), plan.shard.count
        controls, commands = self._spline_commands(plan, b, st)
        pb, policy_out = self._carried(M * N)
        nx = self.plants.nq + self.plants.nv
        states, sensors = pb.rollout_plants(self.plants, b.x0, nx, 1, M, list(range(M)), commands.repeat(M, 1, 1), policy_out, cutoff_time=self.rollout_cutoff_time)
        rows = self._member_cost_rows(N)
        for m in range(M):  # the reward per member, in the shapes a plain controller gives it
            self._score_rollout(states[m * N : (m + 1) * N], sensors[m * N : (m + 1) * N], controls, out=rows[m])
        self.last_rollout = (states[:N], sensors[:N], controls)  # member 0, the nominal plant
        costs = torch.empty(N, dtype=torch.float32, device=self.device)
        self._aggregate(rows, M, N, costs, st.stream)  # (`jh_ensemble_costs`, or its weighted form while plant weights are set)
        return costs


class SpotRandomizedController(Assignment, _SpotPlantController):
    """A Spot `Controller` whose iteration rolls block g of its candidates out on plant `assignment[g]` and updates on the N costs as they are.  `assignment` (G plant
    indices, default g % M) may be set between plan steps -- it travels in the kernel arguments; `plant_of_rollout` and `plant_rewards()` say which plant a reward
    belongs to, and `set_member(b, description)` replaces one plant.  The carried policy outputs and warm start are the controller's own N rows."""

    _kind = "randomised"
    _other_maker = "randomized.make_randomized_controller"

    def __init__(self, controller_config: ControllerConfig, task: Task, optimizer, descriptions: Sequence[dict], blocks: int | None = None,
                 weights: Sequence[float] | None = None, device: torch.device | None = None) -> None:
        self._init_assignment(blocks, weights, len(descriptions))
        super().__init__(controller_config, task, optimizer, descriptions, device=device)

    def _materialised_costs(self, plan, b, st) -> torch.Tensor:
        N, a = plan.shard.count, list(self._assignment)
        controls, commands = self._spline_commands(plan, b, st)
        if self._last_policy_output is None:
            self._last_policy_output = torch.zeros((N, POLICY_OUTPUT_DIM), dtype=torch.float32, device=self.device)
        nx = self.plants.nq + self.plants.nv
        states, sensors = self.rollout_backend.rollout_plants(self.plants, b.x0, nx, 1, len(a), a, commands, self._last_policy_output, cutoff_time=self.rollout_cutoff_time)
        self._assignment_used = a
        return self._score_rollout(states, sensors, controls)


def make_spot_ensemble_controller(task: str | Task, optimizer: str, descriptions: Sequence[dict], worst: int | None = None,
                                  device: torch.device | None = None) -> SpotEnsembleController:
    """`make_controller` for one Spot controller over M plants: the registered task and optimizer (with the task's overrides) around `descriptions`, M descriptions of the
    task's model (`models.scaled_description(task.desc, body_mass=..., geom_friction=..., actuator_kp=...)`).  Member 0 is the nominal plant.  `worst`: how many of a
    candidate's largest member costs are averaged; None: all M, the mean."""
    return make_for(SpotEnsembleController, task, optimizer, descriptions, worst=worst, device=device)


def make_spot_randomized_controller(task: str | Task, optimizer: str, descriptions: Sequence[dict], blocks: int | None = None, weights: Sequence[float] | None = None,
                                    device: torch.device | None = None) -> SpotRandomizedController:
    """`make_controller` for one Spot controller whose candidates are spread over M plants.  `blocks`: the number G of rollout blocks, None: M; `weights`: M non-negative
    numbers that `randomized.blocks_from_weights` turns into the assignment, None: block g on plant g % M.  G must divide `num_rollouts` at the plan step."""
    return make_for(SpotRandomizedController, task, optimizer, descriptions, blocks=blocks, weights=weights, device=device)


__all__ = ["MAX_TREE_PLANTS", "SpotEnsembleController", "SpotRandomizedController", "check_tree_descriptions", "make_spot_ensemble_controller",
           "make_spot_randomized_controller"]
