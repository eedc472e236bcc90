"""B controllers of one model planned in ONE launch (`jh_plan_step_batch` / `jh_plan_step_batch_models`, include/judo_amd.h).

The reference runs one `Controller.update_action` (judo/controller/controller.py:210-299) per process; somebody with several robots, several goals or a
domain-randomised sweep runs B of them back to back and pays B launch chains and B host round trips for work that fits the GPU at once.  A `ControllerFleet`
holds B ordinary `Controller` objects that share one `GpuModel`.  `fleet.update_action()` runs every member's host prelude (time shift, normaliser,
`pre_optimization`, the packed block x0 | nominal | sigma | task params | bounds, the noise) into the member's slice of the fleet's buffers, then ONE
`jh_plan_step_batch` and one `jh_download_end`, then every member's epilogue (denormalise, CEM sigma refit, `update_spline`, the staged trace records).
Afterwards each member is bit for bit where its own `update_action()` would have left it: the kernels run the single plan step's code on offset pointers.

What the members must share is what the launch shares: the model's structure, N, K, H, the spline order, the trace count, the optimizer kind and its scalar arguments.
Everything else -- state, time, goal and the other task parameters, seed or injected noise, CEM sigma -- is a member's own.  So are the model's PHYSICS: members whose
packed images differ in the float section alone (masses, inertias, friction, gains: `models.scaled_description`, `make_controller_fleet(..., descriptions=...)`) keep
their own `GpuModel`, and the fleet plans them through one `GpuModelSet` and `jh_plan_step_batch_models`, a model image per problem.  The header and the int section
of the image (dimensions, topology, pair lists), the kernel build and the self-collision setting stay shared.

The Spot policy tasks have no `GpuModel` and no one-call plan step: their iteration is spline -> command mapping -> policy + plant rollout -> `Task.reward` -> update.  A fleet
of them runs that chain ONCE for the B * n rollouts of its members (`jh_spline_controls_batch`, `jh_policy_rollout_batch`, `jh_update_fused_batch`) around one
`SpotTreeEngine`, one `SpotLocomotionPolicy` and a `PolicyRolloutBackend` of B * n threads; only the rewards stay per member, each task's own `reward` with its own
configuration on its rows.  A rollout's bits depend neither on its wave-mates nor on the batch size (tests/test_gpu_spot.py), so the contract is the same: bit for bit.
"""

from __future__ import annotations

import ctypes as C
import weakref
from typing import Any, Sequence

import numpy as np
import torch

from judo_amd import _lib
from judo_amd.controller import POLICY_OUTPUT_DIM, Controller, make_controller_for
from judo_amd.device import GpuModelSet, current_stream_ptr
from judo_amd.distributed import world_info
from judo_amd.ensemble import EnsembleController
from judo_amd.randomized import RandomizedController
from judo_amd.models import image_sections, layout
from judo_amd.optimizers import Optimizer, _NoiseStream
from judo_amd.tasks import get_registered_tasks


def refuse_fr3_randomized(i: int, c: Controller, fleet: "ControllerFleet | None" = None) -> None:
    """Only an `FR3RandomizedFleet` takes an `FR3RandomizedController` (judo_amd.fr3_randomized) and only an `FR3EnsembleFleet` an `FR3EnsembleController`
    (judo_amd.fr3_ensemble): raises ValueError naming why and the fleet that serves the member.  Every fleet's `_check_member` begins with it."""
    if getattr(c, "_fr3_randomized", False) and not getattr(fleet, "_fr3_randomized_members", False):
        raise ValueError(f"fleet member {i} is an FR3RandomizedController: its plan step (jh_plan_step_randomized_phase) puts the rollout blocks of ONE arm on the launch's "
                         "problem axis, and this fleet's entry has no controller axis behind an arm's rollout blocks.  Randomised fr3_pick controllers share a launch in an "
                         "FR3RandomizedFleet (judo_amd.fr3_randomized_fleet.make_fr3_randomized_fleet); fleets of fr3_pick controllers that believe one plant each are an "
                         "FR3Fleet or an FR3PlantFleet (judo_amd.fr3_fleet.make_fr3_fleet)")
    if getattr(c, "_fr3_ensemble", False) and not getattr(fleet, "_fr3_ensemble_members", False):
        raise ValueError(f"fleet member {i} is an FR3EnsembleController: its plan step (jh_plan_step_ensemble_phase) puts the M plants of ONE arm on the launch's problem "
                         "axis, and this fleet's entry has no controller axis behind an arm's plants.  fr3_pick ensemble controllers share a launch in an FR3EnsembleFleet "
                         "(judo_amd.fr3_ensemble.make_fr3_ensemble_fleet)")
    if getattr(c, "_spot_plants", False):
        raise ValueError(f"fleet member {i} is a {type(c).__name__} (judo_amd.spot_plants): its rollouts run on the plants of its own SpotPlantSet "
                         "(jh_policy_rollout_plants), and a fleet's one policy rollout runs every member's rows on ONE model image -- it would plan this member on plant 0 "
                         "alone.  No fleet takes such a member yet: run its update_action() on its own")
    if getattr(c, "_materialized_plants", False):
        raise ValueError(f"fleet member {i} is a {type(c).__name__} (judo_amd.materialized): its rollouts are materialised on the plants of its own GpuModelSet "
                         "(jh_rollout_materialize_plants) and scored by Task.reward, and a fleet's one launch runs the fused cost of every member on ONE plant each -- it "
                         "would plan this member on plant 0 alone.  No fleet takes such a member yet: run its update_action() on its own")


class _MemberBuffers:
    """A member's slice of the fleet's buffers under the names `Controller`'s helpers use on a `_PlanBuffers`."""

    def __init__(self, fleet: "_FleetBuffers", i: int) -> None:
        f = fleet
        self.sizes, self.offsets = f.sizes, f.offsets
        nblk = f.nblk  # (the five sections: a fleet's extra words lie behind them, inside the stride, and are the fleet's to write)
        self.host_np = f.host_np[i * f.blk_stride : i * f.blk_stride + nblk]
        self.host_ptr, self.nblk_bytes = f.host_ptr + 4 * i * f.blk_stride, 4 * nblk
        self.blk = f.blk[i * f.blk_stride : i * f.blk_stride + nblk]
        self.x0, self.nominal, self.sigma, self.tp, self.lohi = torch.split(self.blk, self.sizes)
        self.blk_stale = True
        self.costs = f.costs[0][i]
        self.dev = f.dev
        # the trace stage of a member whose kernel writes no trace rows (the elites' knots, re-rolled when the traces are read): its own small buffers, made when first needed
        self._fleet, self._i = f, i
        self.trace_rows, self.trace_flip = None, 0
        self._scratch, self._trace_recs = None, None

    @property
    def out_np(self) -> np.ndarray:  # (the fleet's output block may be re-sized between plan steps)
        f = self._fleet
        return f.out_np[self._i * f.out_stride : (self._i + 1) * f.out_stride]

    @property
    def scratch(self) -> torch.Tensor:
        if self._scratch is None:
            f = self._fleet
            self._scratch = torch.empty(int(_lib.lib().jh_update_scratch_floats(f.N, f.K, f.nu)), dtype=torch.float32, device=self.dev)
        return self._scratch

    @property
    def trace_recs(self) -> list[torch.Tensor]:
        if self._trace_recs is None:
            f = self._fleet
            self._trace_recs = [torch.full((max(f.E, 1) * (2 + f.K * f.nu),), float("inf"), dtype=torch.float32, device=self.dev) for _ in range(2)]
        return self._trace_recs


class _FleetBuffers:
    """Everything a fleet's plan step touches, for B problems of one size: B packed blocks in one pinned host buffer (and its device copy), the noise, costs,
    trace rows, update scratch, and the pinned output block with its completion word.  `extra`: words of every block behind `bounds` that belong to the fleet, not to
    the member's five sections (FR3Fleet: the phase word); a member's views end in front of them.  `extra_at`: where in those words the records begin whose offsets the
    fleet's entry takes behind the bounds' (the phase word at 0; a weighted fleet's risk record behind it)."""

    def __init__(self, dev: torch.device, B: int, N: int, K: int, nu: int, nx: int, ntp: int, E: int, extra: int = 0, extra_at: Sequence[int] = (0,)) -> None:
        L = _lib.lib()
        self.dev, self.B, self.N, self.K, self.nu, self.E = dev, B, N, K, nu, E
        self.sizes = [nx, K * nu, K * nu, ntp, 2 * nu]
        self.nblk = sum(self.sizes)
        self.offsets = [int(v) for v in np.cumsum([0] + self.sizes)]
        self.extra = extra
        self.extra_offsets = tuple(self.nblk + int(at) for at in extra_at) if extra else ()  # float offsets in a block, as the entry takes them
        self.blk_stride = self.nblk + extra  # floats from a member's block to the next one's
        self.host = torch.zeros(B * self.blk_stride, dtype=torch.float32).pin_memory()
        self.host_np, self.host_ptr = self.host.numpy(), self.host.data_ptr()
        self.blk = torch.zeros(B * self.blk_stride, dtype=torch.float32, device=dev)
        self.noise = [torch.empty((B, K, nu, N), dtype=torch.float32, device=dev) for _ in range(2)]  # alternated: the other one backs the members' lazy `candidate_knots`
        self.noise_cur = 0
        self.costs = [torch.empty((B, N), dtype=torch.float32, device=dev) for _ in range(2)]  # alternated likewise (`rewards` is read lazily)
        self.scratch = torch.zeros(int(L.jh_plan_batch_scratch_floats(B, N, K, nu)), dtype=torch.float32, device=dev)  # (zero: the tickets)
        self.done = torch.zeros(4, dtype=torch.int32).pin_memory()
        self.trace_buf: torch.Tensor | None = None
        # member i's view of either noise and cost buffer, and of the trace buffer once it exists: made once, not in every iteration (a tensor view costs a microsecond)
        self.noise_rows, self.cost_rows, self.trace_rows = [list(n) for n in self.noise], [list(c) for c in self.costs], []
        self.out_stride = 0
        self.size_out(2 * K * nu)
        self.members = [_MemberBuffers(self, i) for i in range(B)]
        # the launch's argument record, kept from plan step to plan step.  It holds the addresses of `host`, `blk`, `scratch` and `done`: none of them may be reassigned
        # once it exists (`out_host` may: `size_out` replaces it, and the record reads it afresh in every iteration)
        self.step = _LaunchStep(self)

    def size_out(self, stride: int) -> None:
        if self.out_stride >= stride:
            return
        self.out_stride = stride
        self.out_host = torch.zeros(self.B * stride, dtype=torch.float32).pin_memory()  # (zeros: MPPI / PS never write the sigma region)
        self.out_np, self.out_host_ptr = self.out_host.numpy(), self.out_host.data_ptr()


class _LaunchStep:
    """One iteration's library call on a fleet's buffers, as `ControllerFleet._launch` takes it.  It lives with the buffers (`_FleetBuffers.step`), so that the runs of
    arguments every batched plan-step entry shares (include/judo_amd.h) are tuples kept from launch to launch.  The loop assigns by name what a plan step decides --
    `model_set`; `in_place` (the kernel reads the host blocks in place and the host polls the completion word, else the blocks are uploaded and the stream's event kept)
    with `block = blocks[in_place]`; `sizes` (W, N, H, K); `update_args` (mode, lam, k_el, tie); `nfl` (trace floats per step the rollout kernel writes into
    `fb.trace_buf`, 0: none); `colmajor`; `stream` -- and calls `iteration` for the rest.  An entry's call reads: its handle and B / M, `*block`, `*noise_args`, `*sizes`,
    its own middle arguments, `*update_args`, `*tail`."""

    __slots__ = ("fb", "blocks", "model_set", "in_place", "block", "sizes", "update_args", "nfl", "colmajor", "stream", "noise", "costs", "E_t", "row", "noise_args", "tail", "_fixed")

    def __init__(self, fb: "_FleetBuffers") -> None:
        self.fb = fb
        # the blocks: device (or host, read in place), host, bytes of one, bytes from one to the next, the offsets of nominal, sigma, task params and bounds -- and of the
        # fleet's extra words behind the bounds where the blocks have some (the fr3 entries' phase word, the weighted fleets' risk record)
        run = (fb.host_ptr, 4 * (fb.nblk + fb.extra), 4 * fb.blk_stride, *fb.offsets[1:5], *fb.extra_offsets)
        self.blocks = {False: (fb.blk.data_ptr(), *run), True: (fb.host_ptr, *run)}
        self._fixed = (fb.N, fb.K * fb.nu * fb.N, fb.scratch.data_ptr(), fb.done.data_ptr())

    def iteration(self, noise: torch.Tensor, costs: torch.Tensor, E_t: int, row: int) -> None:
        """This iteration's (B, K, nu, N) noise and (B, N) costs, and the `E_t` trace elites' records of `row` floats behind every problem's nominal | sigma -- with the
        output block as the loop has sized it: the tail is update scratch, output block, its stride, the completion mark, no timing events, the stream."""
        fb, (n, pitch, scratch_p, done_p) = self.fb, self._fixed
        self.noise, self.costs, self.E_t, self.row = noise, costs, E_t, row
        self.noise_args = (noise.data_ptr(), n, pitch)
        self.tail = (scratch_p, fb.out_host_ptr, fb.out_stride, done_p if self.in_place else fb.out_host_ptr, None, self.stream)


class ControllerFleet:
    """B controllers of one task and optimizer kind whose plan steps run as one launch.  `fleet[i]` is an ordinary `Controller`: `update_states`,
    `system_metadata`, `optimizer.seed`, `optimizer.injected_noise`, `action(t)`, `traces`, `rewards` work per member as they do on a controller alone.

    `update_action` is the one loop of every fleet whose iteration is a library call; a subclass with another call (`judo_amd.ensemble_fleet.EnsembleFleet`) replaces
    `_check_member`, `_models`, `_trace_floats` and `_launch` and keeps the loop."""

    _ensemble_members = False  # members are `EnsembleController`s, each planning against M plants (EnsembleFleet)
    _randomized_members = False  # members are `RandomizedController`s, each spreading its rollout blocks over the M plants of its set (RandomizedFleet)
    _fr3_members = False  # members are fr3_pick controllers, whose phase travels in the packed block (judo_amd.fr3_fleet.FR3Fleet)
    _block_extra_words = 0  # words of every packed block behind the bounds that the fleet writes itself (FR3Fleet: 1, the phase word)
    _block_extra_at: tuple = (0,)  # where in those words the records begin whose offsets the entry takes (judo_amd.weighted_fleet: the risk record, behind the phase word if any)

    def __init__(self, controllers: Sequence[Controller]) -> None:
        self.controllers = list(controllers)
        if not self.controllers:
            raise ValueError("a fleet needs at least one controller")
        first = self.controllers[0]
        self.device = first.device
        for i, c in enumerate(self.controllers):
            self._check_member(i, c, first)
        self.model = first.model
        self.policy_backend = None  # the Spot policy tasks: the fleet's own backend of B * n threads around the members' one engine and one policy
        if first.task.uses_locomotion_policy:
            for i, c in enumerate(self.controllers):  # (a member's carried state becomes a view of THIS fleet's tensors, _load_carry: a controller is in one fleet at a time)
                other = getattr(c, "_fleet_ref", lambda: None)()
                if other is not None and other is not self:
                    raise ValueError(f"fleet member {i} already belongs to another ControllerFleet: a Spot controller is a member of at most one fleet at a time")
                c._fleet_ref = weakref.ref(self)
            for c in self.controllers[1:]:  # one model image and one copy of the actor weights on the device for the whole fleet
                c.rollout_backend.engine, c.rollout_backend.policy = first.rollout_backend.engine, first.rollout_backend.policy
            self._policy_out: torch.Tensor | None = None  # (B * n, 12): the members' `_last_policy_output` are views of it
        for c in self.controllers[1:]:  # one image of the model constants on the device for every member whose image is member 0's, byte for byte
            if not (self._ensemble_members or self._randomized_members) and c.model is not self.model and c.model._blob == self.model._blob:
                c.model = c.task._gpu = c.rollout_backend.model = self.model
        self._model_set: GpuModelSet | None = None  # members with images of their own (randomised physics): their float sections side by side, made at the first plan step
        self._bufs: _FleetBuffers | None = None
        self._bufs_key: tuple | None = None

    def __len__(self) -> int:
        return len(self.controllers)

    def __getitem__(self, i: int) -> Controller:
        return self.controllers[i]

    def __iter__(self):
        return iter(self.controllers)

    # ---- what a member must share with the fleet ---------------------------------------------------------------------------------------------------
    @staticmethod
    def _shared(c: Controller) -> dict[str, Any]:
        opt = c.optimizer
        return {"task class": type(c.task), "optimizer class": type(opt), "num_rollouts": opt.num_rollouts, "num_nodes": opt.num_nodes, "horizon": c.horizon,
                "spline_order": c.spline_order, "max_num_traces": c.max_num_traces, "max_opt_iters": c.max_opt_iters,
                "fused_update_args": opt.fused_update_args() if hasattr(opt, "fused_update_args") else None}

    @staticmethod
    def _shared_policy(c: Controller) -> dict[str, Any]:
        """What the members of a Spot fleet share beyond `_shared`: what the one rollout launch chain and the one command mapping take from member 0."""
        t, rb = c.task, c.rollout_backend
        return {"physics_substeps": rb.physics_substeps, "rollout_cutoff_time": c.rollout_cutoff_time, "carry_warmstart": rb.carry_warmstart, "self_collision": rb.engine.self_collision,
                "use_arm": t.use_arm, "use_gripper": t.use_gripper, "use_legs": t.use_legs, "use_torso": t.use_torso, "command_mask": t.command_mask.tolist(),
                "default_policy_command": np.asarray(t.default_policy_command).tolist()}

    def _check_member(self, i: int, c: Controller, first: Controller) -> None:
        refuse_fr3_randomized(i, c, self)
        if isinstance(c, RandomizedController) and not self._randomized_members:
            # (its iteration shape reads "plan_step" too, and the batched plan step would run every block on `c.model`, plant 0, and drop the assignment without a word)
            raise ValueError(f"fleet member {i} is a RandomizedController: its plan step spreads the rollout blocks over the plants of its own set "
                             "(jh_plan_step_randomized), which a ControllerFleet's launch does not do; randomised controllers share a launch in a RandomizedFleet "
                             "(judo_amd.randomized_fleet.make_randomized_fleet)")
        if isinstance(c, EnsembleController) and not self._ensemble_members:
            # (its iteration shape reads "plan_step", but the batched plan step would run on `c.model`, plant 0 alone, and drop the ensemble without a word)
            raise ValueError(f"fleet member {i} is an EnsembleController: a ControllerFleet plans every member on one plant; ensemble controllers share a launch in an "
                             "EnsembleFleet (judo_amd.ensemble_fleet.make_ensemble_fleet)")
        if c.model is not None and c.model.desc.get("family", c.model.task) == "fr3_pick" and not self._fr3_members:
            raise ValueError(f"fleet member {i}: fr3_pick has no batched plan step (its phase is chosen per problem on the host) in a ControllerFleet: fr3_pick controllers "
                             "share a launch in an FR3Fleet (judo_amd.fr3_fleet.make_fr3_fleet)")
        if c.device != first.device:
            raise ValueError(f"fleet member {i} is on {c.device}, the fleet on {first.device}")
        mine, want = self._shared(c), self._shared(first)
        for key in want:
            if mine[key] != want[key]:
                raise ValueError(f"fleet member {i} differs from member 0 in {key}: {mine[key]!r} against {want[key]!r}")
        policy = c.task.uses_locomotion_policy
        if policy:
            mine, want = self._shared_policy(c), self._shared_policy(first)
            for key in want:
                if mine[key] != want[key]:
                    raise ValueError(f"fleet member {i} differs from member 0 in {key}: {mine[key]!r} against {want[key]!r}")
            mine_e, want_e = c.rollout_backend.engine, first.rollout_backend.engine
            if mine_e is not want_e and bytes(mine_e._blob) != bytes(want_e._blob):
                raise ValueError(f"fleet member {i} has another model image than member 0")
        elif c.model is not first.model:
            if c.model._blob != first.model._blob:  # images may differ in the float section alone: physics per problem, one structure for the launch
                mine_s, want_s = image_sections(c.model._blob), image_sections(first.model._blob)
                for name, x, y in zip(("header", "float section", "int section"), mine_s, want_s):
                    if (x != y and name != "float section") or len(x) != len(y):
                        raise ValueError(f"fleet member {i} has another model image or kernel build than member 0: the {name} of its image differs")
            if c.model.build() != first.model.build() or c.model.self_collision != first.model.self_collision:
                raise ValueError(f"fleet member {i} has another model image or kernel build than member 0: the kernel build or the self-collision setting differs")
        world, _ = world_info(c.group)
        nrm = c._current_normalizer()
        shape = c._iteration_shape(world, nrm)
        # a Spot member's iteration is the materialise path without moments ("update_fused"); everybody else's the one jh_plan_step call
        ok = (shape == "update_fused" and not nrm.needs_moments) if policy else shape == "plan_step"
        if not ok or c.keep_candidates or c.record_kernel_events:
            why = ("a process group" if world > 1 or c.force_shard_path else "keep_candidates" if c.keep_candidates else "record_kernel_events" if c.record_kernel_events
                   else "a running normaliser" if nrm.needs_moments else "a plugin reward, hook or optimizer, or a knot count above the fused kernel's limit")
            how = "as spline, policy rollout, reward and jh_update_fused" if policy else "as one jh_plan_step call"
            raise ValueError(f"fleet member {i} does not run its iteration {how} ({why}): only such controllers can share a launch")

    # ---- the plan step --------------------------------------------------------------------------------------------------------------------------------
    def _models(self) -> GpuModelSet | None:
        """None where every member plans on the fleet's one `GpuModel` (`jh_plan_step_batch`); else the set of the members' models, rebuilt when a member's model was
        exchanged between plan steps."""
        models = [c.model for c in self.controllers]
        if all(m is self.model for m in models):
            self._model_set = None
        elif self._model_set is None or len(self._model_set.models) != len(models) or any(a is not b for a, b in zip(self._model_set.models, models)):
            self._model_set = GpuModelSet(models)
        return self._model_set

    def _buffers(self, key: tuple) -> _FleetBuffers:
        if self._bufs_key != key:
            self._bufs, self._bufs_key = _FleetBuffers(self.device, *key, extra=self._block_extra_words, extra_at=self._block_extra_at), key
        return self._bufs

    def _draw_noise(self, fb: _FleetBuffers, N: int, K: int, nu: int) -> torch.Tensor:
        """The members' noise into the next (B, K, nu, N) buffer: one `jh_noise_normal_batch` when every member draws from the device generator (each member's draw
        counter advances by one, as its own `draw_noise` would leave it), else member by member through `draw_noise`."""
        fb.noise_cur ^= 1
        noise = fb.noise[fb.noise_cur]
        opts = [c.optimizer for c in self.controllers]
        if all(o.injected_noise is None and type(o).draw_noise is Optimizer.draw_noise for o in opts):
            B = len(opts)
            for o in opts:
                if o._generator is None:
                    o._generator = _NoiseStream(o._seed)
            seeds = (C.c_ulonglong * B)(*[o._generator.seed for o in opts])
            draws = (C.c_uint * B)(*[o._generator.draws & 0xFFFFFFFF for o in opts])
            _lib.check(_lib.lib().jh_noise_normal_batch(B, seeds, draws, K * nu, N, noise.data_ptr(), N, current_stream_ptr()), "jh_noise_normal_batch")
            for i, o in enumerate(opts):
                o._generator.draws += 1
                o.last_noise = noise[i]
        else:
            for i, o in enumerate(opts):
                got = o.draw_noise(N, 0, self.device, out=noise[i])
                if got.data_ptr() != noise[i].data_ptr():  # (injected noise, or a plugin's own draw: a tensor of its own)
                    noise[i].copy_(got)
                    o.last_noise = noise[i]
        return noise

    def update_action(self) -> None:
        lib = _lib.lib()
        cs = self.controllers
        first = cs[0]
        for i, c in enumerate(cs):  # (live edits of a config between plan steps must not silently split the fleet)
            self._check_member(i, c, first)
        if first.task.uses_locomotion_policy:
            return self._update_action_policy()
        model_set = self._models()
        plans, fb, states = self._begin_plans()
        p0, stream = plans[0], states[0].stream
        N, K, nu, H, E, B = p0.N, p0.K, p0.nu, p0.H, p0.E, len(cs)
        nfl = self._trace_floats()
        in_place = self.model.closed_form  # (the closed-form kernels read the host blocks in place and the host polls the completion word; the leap family uploads and keeps the stream's event)
        step = fb.step
        step.model_set, step.in_place, step.block, step.sizes = model_set, in_place, step.blocks[in_place], (p0.W.data_ptr(), N, H, K)
        step.update_args, step.nfl, step.colmajor, step.stream = first.optimizer.fused_update_args(), nfl, int(first._trace_colmajor) if nfl else 0, stream
        iters, staged = 0, False
        while iters < first.max_opt_iters and not any(c.optimizer.stop_cond() for c in cs):
            last = iters == first.max_opt_iters - 1
            self._member_inputs(plans, fb, states)
            noise = self._draw_noise(fb, N, K, nu)
            costs = fb.costs[fb.noise_cur]
            row = H * nfl
            if nfl and (fb.trace_buf is None or fb.trace_buf.numel() != B * N * row):
                fb.trace_buf = torch.empty(B * N * row, dtype=torch.float32, device=self.device)
                fb.trace_rows = list(fb.trace_buf.view(B, N * row))
            E_t = min(E, _lib.MAX_ELITES) if (last and nfl) else 0
            fb.size_out(2 * K * nu + E_t * (2 + row))
            step.iteration(noise, costs, E_t, row)
            self._launch(step)
            _lib.check(lib.jh_download_end(), "jh_download_end")
            self._member_results(plans, fb, states, in_place, row, E_t, last)
            staged = last
            iters += 1
        self._end_plans(plans, fb, states, iters, staged)

    # ---- what both loops share: the members' host work in front of, inside and behind the iterations ------------------------------------------------------------
    def _begin_plans(self) -> tuple[tuple, _FleetBuffers, tuple]:
        """Every member's `_begin_plan`, the agreement of the problem sizes, the fleet's buffers for them and the launch stream in every member's iteration state."""
        cs = self.controllers
        plans, states = zip(*[c._begin_plan() for c in cs])
        size = None
        for i, p in enumerate(plans):
            mine = (p.N, p.K, p.nu, p.H, p.E, len(p.tp))
            if size is None:
                size = mine
            if mine != size:
                raise ValueError(f"fleet member {i} plans another problem size than member 0")
            assert p.world == 1 and p.shard.count == p.N  # (`_check_member` refused a member with a process group: the members' trace stage calls all_gather_records with no group)
        N, K, nu, _, E, ntp = size
        fb = self._buffers((len(cs), N, K, nu, cs[0].task.nq + cs[0].task.nv, ntp, E))
        stream = current_stream_ptr()
        for st in states:
            st.stream = stream
        return plans, fb, states

    def _member_inputs(self, plans: tuple, fb: _FleetBuffers, states: tuple) -> None:
        """An iteration's host prelude: every member's `pre_rollout` and its packed block, in its slice of the fleet's pinned host block (not uploaded here)."""
        for c, p, mb, st in zip(self.controllers, plans, fb.members, states):
            c._stream = st.stream
            c.task.pre_rollout(c.current_state)
            c._iteration_inputs(p, mb, st, upload=False)

    def _member_results(self, plans: tuple, fb: _FleetBuffers, states: tuple, stale: bool, row: int, E_t: int, last: bool) -> None:
        """Behind an iteration's wait: every member's iteration state as its own iteration would have left it, the update's result read from its slice of the output
        block, and -- in the last iteration, where the update wrote no trace records -- its trace stage (the elites' knots, re-rolled when the traces are read, or
        their rows of the materialised sensors).  The iteration's noise and costs are the buffers `_draw_noise` flipped to.  `stale`: the device copy of the blocks was
        not written; `row`: trace floats per rollout in `fb.trace_buf`, 0: none."""
        N, noise, costs, traces = fb.N, fb.noise_rows[fb.noise_cur], fb.cost_rows[fb.noise_cur], fb.trace_rows
        for i, (c, p, mb, st) in enumerate(zip(self.controllers, plans, fb.members, states)):
            mb.blk_stale = stale
            st.costs = mb.costs = costs[i]
            n_i = st.noise = noise[i]
            st.noise_p, st.ldn = n_i.data_ptr(), N
            st.knots_out = st.knots_nku = None
            st.trace_buf = (traces[i], row) if row else None
            st.stages = last
            c._iteration_result(p, mb, st, E_t)
            if last and not E_t:
                c._stage_traces(p, mb, st)

    def _end_plans(self, plans: tuple, fb: _FleetBuffers, states: tuple, iters: int, staged: bool) -> None:
        for c, p, mb, st in zip(self.controllers, plans, fb.members, states):
            c._end_plan(p, mb, st, iters, staged)

    def _trace_floats(self) -> int:
        """Trace floats per step that the fleet's rollout kernel writes for every rollout; 0: none, and the members re-roll their trace elites when the traces are read."""
        return self.controllers[0]._fused_trace_floats()

    def _launch(self, step: _LaunchStep) -> None:
        """The one library call of an iteration: B plan steps on the fleet's buffers, with the completion mark that `jh_download_end` then waits for."""
        if step.model_set is not None:  # a model image per problem: the same call without B, which the set holds
            self._launch_traced(_lib.lib().jh_plan_step_batch_models, (step.model_set.handle,), step)
        else:
            self._launch_traced(_lib.lib().jh_plan_step_batch, (self.model.handle, len(self.controllers)), step)

    @staticmethod
    def _launch_traced(entry, head: tuple, step: _LaunchStep) -> None:
        """The entries of the controllers that believe one plant each, whose rollout kernel writes the trace rows: `head` (the model or the set, B), then the runs."""
        s = step
        rc = entry(*head, *s.block, *s.noise_args, *s.sizes, s.costs.data_ptr(), s.fb.trace_buf.data_ptr() if s.nfl else None, *s.update_args, s.E_t, s.row, s.colmajor, *s.tail)
        _lib.check(rc, entry.__name__)

    def _write_phases(self, fb: _FleetBuffers) -> None:
        """The fr3 fleets: the members' phases (decided by their `pre_rollout` in this iteration) into the phase words behind their blocks' bounds."""
        for i, c in enumerate(self.controllers):
            fb.host_np[i * fb.blk_stride + fb.nblk] = float(int(c.task.phase))

    # ---- the plan step of the Spot policy tasks ------------------------------------------------------------------------------------------------------
    def _load_carry(self, B: int, n: int) -> torch.Tensor:
        """The fleet's backend of B * n threads, its warm start and the (B * n, 12) policy outputs holding every member's carried state: a member's `_last_policy_output` and
        its backend's warm start are views of its n rows, so what a member brings along from elsewhere -- zeros after `reset()` or `rollout_backend.update()`, its own arrays
        after plan steps on its own -- is copied in here, and what the fleet's rollout leaves is the member's without a copy.  Whether a member's tensor already is its
        view is told from its address and shape, which holds because a Spot controller belongs to at most one fleet at a time (checked in `__init__`)."""
        first = self.controllers[0].rollout_backend
        pb = self.policy_backend
        if pb is None or pb.engine is not first.engine or pb.policy is not first.policy:
            from judo_amd.policy import PolicyRolloutBackend

            pb = self.policy_backend = PolicyRolloutBackend(B * n, physics_substeps=first.physics_substeps, device=self.device, carry_warmstart=first.carry_warmstart, share=first)
        pb.physics_substeps, pb.carry_warmstart = first.physics_substeps, first.carry_warmstart
        if pb.num_threads != B * n:
            pb.update(B * n)
        if self._policy_out is None or self._policy_out.shape[0] != B * n:
            self._policy_out = torch.zeros((B * n, POLICY_OUTPUT_DIM), dtype=torch.float32, device=self.device)
        for i, c in enumerate(self.controllers):
            warm, out = pb._warm[i * n : (i + 1) * n], self._policy_out[i * n : (i + 1) * n]
            mine = c.rollout_backend._warm
            if mine.data_ptr() != warm.data_ptr() or mine.shape != warm.shape:
                warm.copy_(mine)
                c.rollout_backend._warm = warm
            mine = c._last_policy_output
            if mine is None:
                out.zero_()
            elif mine.data_ptr() != out.data_ptr() or mine.shape != out.shape:
                out.copy_(mine)
            c._last_policy_output = out
        return self._policy_out

    def _update_action_policy(self) -> None:
        """`Controller.update_action` of B Spot members (the iteration shape "update_fused": Controller._rollout_update with Controller._materialised_costs) as one launch
        chain per iteration: every stage that runs on the device once per controller there runs once per fleet here."""
        lib = _lib.lib()
        cs = self.controllers
        first = cs[0]
        plans, fb, states = self._begin_plans()
        p0, stream = plans[0], states[0].stream
        N, K, nu, H, W, B = p0.N, p0.K, p0.nu, p0.H, p0.W, len(cs)
        mode, lam, k_el, tie = first.optimizer.fused_update_args()
        off = fb.offsets
        policy_out = self._load_carry(B, N)
        iters, staged = 0, False
        while iters < first.max_opt_iters and not any(c.optimizer.stop_cond() for c in cs):
            last = iters == first.max_opt_iters - 1
            self._member_inputs(plans, fb, states)
            _lib.check(lib.jh_upload_async(fb.blk.data_ptr(), fb.host_ptr, 4 * ((B - 1) * fb.blk_stride + fb.nblk), stream), "jh_upload_async")
            noise = self._draw_noise(fb, N, K, nu)
            costs = fb.costs[fb.noise_cur]
            controls = torch.empty((B * N, H, nu), dtype=torch.float32, device=self.device)  # (fresh arrays per iteration, as the controller alone makes them: `last_rollout` keeps views)
            st = lib.jh_spline_controls_batch(_lib.ptr(W), B, fb.blk.data_ptr(), fb.blk_stride, off[1], off[2], off[4], noise.data_ptr(), N, K * nu * N, N, H, K, nu, controls.data_ptr(), stream)
            _lib.check(st, "jh_spline_controls_batch")
            # the members' `use_*` flags agree (_check_member), so the command mapping is one elementwise pass over all rows (judo/tasks/spot/spot_base.py:325-391)
            commands = first.task.task_to_sim_ctrl(controls).contiguous()
            states_d, sensors_d = self.policy_backend.rollout_grouped(fb.blk, fb.blk_stride, B, commands, policy_out, cutoff_time=first.rollout_cutoff_time)
            for i, c in enumerate(cs):
                r = slice(i * N, (i + 1) * N)
                c._score_rollout(states_d[r], sensors_d[r], controls[r], out=costs[i])
            st = lib.jh_update_fused_batch(B, costs.data_ptr(), fb.blk.data_ptr(), fb.blk_stride, off[1], off[2], off[4], noise.data_ptr(), N, K * nu * N, N, K, nu, mode, lam, k_el, tie,
                                           0, None, 0, 0, fb.scratch.data_ptr(), fb.out_host_ptr, fb.out_stride, fb.out_host_ptr, stream)
            _lib.check(st, "jh_update_fused_batch")
            _lib.check(lib.jh_download_end(), "jh_download_end")
            self._member_results(plans, fb, states, False, 0, 0, last)  # (no trace rows from a kernel: the elites' rows of the materialised sensors, Controller._stage_traces' `last_rollout` branch)
            staged = last
            iters += 1
        self._end_plans(plans, fb, states, iters, staged)

    def solver_stats(self, reset: bool = True) -> dict:
        """`Controller.solver_stats` for the fleet.  The members share one engine (one `GpuModel`, or one `SpotTreeEngine`) and the counters live on it: they are fleet-wide,
        and a member's own `solver_stats()` reads -- and resets -- the same fleet-wide counters, not that member's share.  A fleet with a model image per member counts its
        launches on member 0's model too."""
        return self.controllers[0].solver_stats(reset)


def make_controller_fleet(task: str, optimizer: str, B: int, device: torch.device | None = None, descriptions: Sequence[dict] | None = None) -> ControllerFleet:
    """B controllers of the registered task and optimizer (`make_controller`, judo/controller/controller.py:404-442, B times) around ONE `GpuModel` -- or, for the Spot
    policy tasks, ONE `SpotTreeEngine` and ONE `SpotLocomotionPolicy`.

    `descriptions`: B model descriptions, one per member (randomised physics: `models.scaled_description(task.desc, body_mass=..., geom_friction=..., actuator_kp=...)`).
    Member i's task takes `descriptions[i]` before its first device use and keeps a `GpuModel` of its own; the fleet still plans in one launch, a model image per problem.
    The descriptions must pack to images that differ in the float section alone; the Spot policy tasks and fr3_pick take none."""
    tasks = get_registered_tasks()
    if task not in tasks:
        raise ValueError(f"Task {task} not found in task registry.")
    if B < 1:
        raise ValueError("a fleet needs at least one controller")
    if descriptions is not None and len(descriptions) != B:
        raise ValueError(f"{len(descriptions)} descriptions for a fleet of {B}")
    members: list[Controller] = []
    for i in range(B):
        t = tasks[task][0]()
        share = None
        if descriptions is not None:
            if t.uses_locomotion_policy:
                raise ValueError("a Spot fleet is one policy rollout over all members' rows and shares one model image: it takes no per-member descriptions")
            t.desc = descriptions[i]
            t._layout, t._ctrlrange, t._jadr = layout(t.desc), None, None
            if members and t.desc is members[0].task.desc:
                t._gpu = members[0].model
        elif members and t.uses_locomotion_policy:
            share = members[0].rollout_backend  # (Controller builds its PolicyRolloutBackend around that one's engine and policy)
        elif members:
            t._gpu = members[0].model  # (Task.gpu_model hands it out instead of packing and uploading the image again)
        members.append(make_controller_for(t, optimizer, device=device, policy_share=share))
    return ControllerFleet(members)
