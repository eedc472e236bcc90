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
    the member's five sections (FR3Fleet: the phase word); a member's views end in front of them."""

    def __init__(self, dev: torch.device, B: int, N: int, K: int, nu: int, nx: int, ntp: int, E: int, extra: int = 0) -> None:
        L = _lib.lib()
        self.dev, self.B, self.N, self.K, self.nu, self.E = dev, B, N, K, nu, E
        self.sizes = [nx, K * nu, K * nu, ntp, 2 * nu]
        self.nblk = sum(self.sizes)
        self.offsets = [int(v) for v in np.cumsum([0] + self.sizes)]
        self.extra = extra
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
        self.out_stride = 0
        self.size_out(2 * K * nu)
        self.members = [_MemberBuffers(self, i) for i in range(B)]

    def size_out(self, stride: int) -> None:
        if self.out_stride >= stride:
            return
        self.out_stride = stride
        self.out_host = torch.zeros(self.B * stride, dtype=torch.float32).pin_memory()  # (zeros: MPPI / PS never write the sigma region)
        self.out_np, self.out_host_ptr = self.out_host.numpy(), self.out_host.data_ptr()


class ControllerFleet:
    """B controllers of one task and optimizer kind whose plan steps run as one launch.  `fleet[i]` is an ordinary `Controller`: `update_states`,
    `system_metadata`, `optimizer.seed`, `optimizer.injected_noise`, `action(t)`, `traces`, `rewards` work per member as they do on a controller alone.

    `update_action` is the one loop of every fleet whose iteration is a library call; a subclass with another call (`judo_amd.ensemble_fleet.EnsembleFleet`) replaces
    `_check_member`, `_models`, `_trace_floats` and `_launch` and keeps the loop."""

    _ensemble_members = False  # members are `EnsembleController`s, each planning against M plants (EnsembleFleet)
    _randomized_members = False  # members are `RandomizedController`s, each spreading its rollout blocks over the M plants of its set (RandomizedFleet)
    _fr3_members = False  # members are fr3_pick controllers, whose phase travels in the packed block (judo_amd.fr3_fleet.FR3Fleet)
    _block_extra_words = 0  # words of every packed block behind the bounds that the fleet writes itself (FR3Fleet: 1, the phase word)

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
            self._bufs, self._bufs_key = _FleetBuffers(self.device, *key, extra=self._block_extra_words), key
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
        plans = [c._begin_plan() for c in cs]
        # (a plan: N, K, nu, H, world, shard, normaliser, normalised nominal, W, x0, new knot times, fused optimizer?, trace elites, task params -- Controller._begin_plan)
        N, K, nu, H, _, _, _, _, W, _, _, _, E, tp0 = plans[0]
        for i, p in enumerate(plans):
            if (p[0], p[1], p[2], p[3], p[12], len(p[13])) != (N, K, nu, H, E, len(tp0)):
                raise ValueError(f"fleet member {i} plans another problem size than member 0")
        B = len(cs)
        fb = self._buffers((B, N, K, nu, first.task.nq + first.task.nv, len(tp0), E))
        stream = current_stream_ptr()
        shards, nrms = [p[5] for p in plans], [p[6] for p in plans]
        states: list[dict[str, Any]] = [dict(E=E, x0=p[9], new_times=p[10]) for p in plans]
        nominal_n = [p[7] for p in plans]
        mode, lam, k_el, tie = first.optimizer.fused_update_args()
        nfl = self._trace_floats()
        colmajor = int(first._trace_colmajor) if nfl else 0
        iters, staged = 0, False
        while iters < first.max_opt_iters and not any(c.optimizer.stop_cond() for c in cs):
            last = iters == first.max_opt_iters - 1
            affine = []
            for c, mb, nrm, n_n in zip(cs, fb.members, nrms, nominal_n):
                c._stream = stream
                c.task.pre_rollout(c.current_state)
                affine.append(c._iteration_inputs(mb, nrm, n_n, nu, upload=False))
            noise = self._draw_noise(fb, N, K, nu)
            costs = fb.costs[fb.noise_cur]
            row = H * nfl
            if nfl and (fb.trace_buf is None or fb.trace_buf.numel() != B * N * row):
                fb.trace_buf = torch.empty(B * N * row, dtype=torch.float32, device=self.device)
            E_t = min(E, _lib.MAX_ELITES) if (last and nfl) else 0
            fb.size_out(2 * K * nu + E_t * (2 + row))
            in_place = self.model.closed_form  # (the closed-form kernels read the host blocks in place and the host polls the completion word; the leap family uploads and keeps the stream's event)
            self._launch(lib, model_set, fb, in_place, noise, W, N, H, K, nu, costs, nfl, (mode, lam, k_el, tie), E_t, row, colmajor, stream)
            _lib.check(lib.jh_download_end(), "jh_download_end")
            for i, (c, mb, shard, st_i) in enumerate(zip(cs, fb.members, shards, states)):
                mb.blk_stale = in_place
                mb.costs = costs[i]
                trace_i = (fb.trace_buf[i * N * row : (i + 1) * N * row], row) if nfl else None
                st_i.update(costs=mb.costs, knots_out=None, noise_p=noise[i].data_ptr(), ldn=N, knots_nku=None, trace_buf=trace_i, stage=(True if last else None))
                nominal_n[i] = c._iteration_result(mb, st_i, noise[i], noise[i].data_ptr(), N, shard, H, K, nu, E_t, *affine[i])
                if last and not E_t:  # (no trace rows from the kernel: the elites' knots, re-rolled when the traces are read)
                    c._stage_traces(lib, mb, st_i, shard, 1, E, st_i["x0"], st_i["new_times"], K, nu, stream)
            staged = last
            iters += 1
        for c, mb, p, st_i, n_n in zip(cs, fb.members, plans, states, nominal_n):
            c._end_plan(p, mb, st_i, n_n, iters, staged, stream)

    def _trace_floats(self) -> int:
        """Trace floats per step that the fleet's rollout kernel writes for every rollout; 0: none, and the members re-roll their trace elites when the traces are read."""
        return self.controllers[0]._fused_trace_floats()

    def _launch(self, lib, model_set: GpuModelSet | None, fb: _FleetBuffers, in_place: bool, noise: torch.Tensor, W, N: int, H: int, K: int, nu: int, costs: torch.Tensor, nfl: int,
                update_args: tuple, E_t: int, row: int, colmajor: int, stream) -> None:
        """The one library call of an iteration: B plan steps on the fleet's buffers, with the completion mark that `jh_download_end` then waits for."""
        B = len(self.controllers)
        off = fb.offsets
        mode, lam, k_el, tie = update_args
        if model_set is not None:  # a model image per problem: the same call without the model and B, which the set holds
            st = lib.jh_plan_step_batch_models(model_set.handle, fb.host_ptr if in_place else fb.blk.data_ptr(), fb.host_ptr, 4 * fb.nblk, 4 * fb.blk_stride, off[1], off[2], off[3], off[4],
                                               noise.data_ptr(), N, K * nu * N, _lib.ptr(W), N, H, K, costs.data_ptr(), fb.trace_buf.data_ptr() if nfl else None, mode, lam, k_el, tie,
                                               E_t, row, colmajor, fb.scratch.data_ptr(), fb.out_host_ptr, fb.out_stride, fb.done.data_ptr() if in_place else fb.out_host_ptr, None, stream)
            _lib.check(st, "jh_plan_step_batch_models")
        else:
            st = lib.jh_plan_step_batch(self.model.handle, B, fb.host_ptr if in_place else fb.blk.data_ptr(), fb.host_ptr, 4 * fb.nblk, 4 * fb.blk_stride, off[1], off[2], off[3], off[4],
                                        noise.data_ptr(), N, K * nu * N, _lib.ptr(W), N, H, K, costs.data_ptr(), fb.trace_buf.data_ptr() if nfl else None, mode, lam, k_el, tie, E_t,
                                        row, colmajor, fb.scratch.data_ptr(), fb.out_host_ptr, fb.out_stride, fb.done.data_ptr() if in_place else fb.out_host_ptr, None, stream)
            _lib.check(st, "jh_plan_step_batch")

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
        plans = [c._begin_plan() for c in cs]
        N, K, nu, H, _, _, _, _, W, _, _, _, E, tp0 = plans[0]
        for i, p in enumerate(plans):
            if (p[0], p[1], p[2], p[3], p[12], len(p[13])) != (N, K, nu, H, E, len(tp0)):
                raise ValueError(f"fleet member {i} plans another problem size than member 0")
        B = len(cs)
        fb = self._buffers((B, N, K, nu, first.task.nq + first.task.nv, len(tp0), E))
        stream = current_stream_ptr()
        shards, nrms = [p[5] for p in plans], [p[6] for p in plans]
        states: list[dict[str, Any]] = [dict(E=E, x0=p[9], new_times=p[10]) for p in plans]
        nominal_n = [p[7] for p in plans]
        mode, lam, k_el, tie = first.optimizer.fused_update_args()
        off = fb.offsets
        policy_out = self._load_carry(B, N)
        iters, staged = 0, False
        while iters < first.max_opt_iters and not any(c.optimizer.stop_cond() for c in cs):
            last = iters == first.max_opt_iters - 1
            affine = []
            for c, mb, nrm, n_n in zip(cs, fb.members, nrms, nominal_n):
                c._stream = stream
                c.task.pre_rollout(c.current_state)
                affine.append(c._iteration_inputs(mb, nrm, n_n, nu, upload=False))
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
            for i, (c, mb, shard, st_i) in enumerate(zip(cs, fb.members, shards, states)):
                mb.blk_stale = False
                mb.costs = costs[i]
                st_i.update(costs=mb.costs, knots_out=None, noise_p=noise[i].data_ptr(), ldn=N, knots_nku=None, trace_buf=None, stage=(True if last else None))
                nominal_n[i] = c._iteration_result(mb, st_i, noise[i], noise[i].data_ptr(), N, shard, H, K, nu, 0, *affine[i])
                if last:  # (the trace elites' rows of the materialised sensors, Controller._stage_traces' `last_rollout` branch)
                    c._stage_traces(lib, mb, st_i, shard, 1, E, st_i["x0"], st_i["new_times"], K, nu, stream)
            staged = last
            iters += 1
        for c, mb, p, st_i, n_n in zip(cs, fb.members, plans, states, nominal_n):
            c._end_plan(p, mb, st_i, n_n, iters, staged, stream)

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
