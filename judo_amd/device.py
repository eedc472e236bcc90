"""Device plumbing: PyTorch-ROCm is used only as the container for device memory, streams and RCCL.

`GpuModel` owns one `jh_model` handle (model constants resident in HBM) per (task, device); `GpuModelSet` one `jh_model_set`: the float sections of B models of one
structure side by side, for a batched plan step with a model image per problem.
"""

from __future__ import annotations

import ctypes as C
import os

import numpy as np
import torch

from judo_amd import _lib
from judo_amd.models import layout, load_description, pack_model


def require_gpu() -> torch.device:
    if not torch.cuda.is_available():
        raise RuntimeError("judo_amd needs an MI355X (HIP device): torch.cuda.is_available() is False and there is no CPU fallback")
    return torch.device("cuda", torch.cuda.current_device())


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def current_stream_ptr() -> int:
    """The current HIP stream of the current device as an integer (what the C ABI takes).  `torch.cuda.current_stream()` builds a Stream object through several
    layers of Python (10 us per call, a tenth of a small plan step); the raw accessor behind it returns the same handle in well under a microsecond."""
    if _raw_stream is not None:
        return int(_raw_stream(torch.cuda.current_device()))
    return torch.cuda.current_stream().cuda_stream


class HipEvent:
    """A timing event on the launch stream (jh_event_*): what `Controller.record_kernel_events` brackets the kernels with.  Same two methods as torch.cuda.Event, but the
    handle exists from construction on, so the library can record it inside a multi-kernel call (jh_plan_step)."""

    __slots__ = ("handle",)

    def __init__(self) -> None:
        h = C.c_void_p()
        _lib.check(_lib.lib().jh_event_create(C.byref(h)), "jh_event_create")
        self.handle = h.value

    def record(self, stream: int | None = None) -> None:
        _lib.check(_lib.lib().jh_event_record(self.handle, current_stream_ptr() if stream is None else stream), "jh_event_record")

    def elapsed_time(self, other: "HipEvent") -> float:
        ms = C.c_float()
        _lib.check(_lib.lib().jh_event_elapsed_ms(self.handle, other.handle, C.byref(ms)), "jh_event_elapsed_ms")
        return float(ms.value)

    def __del__(self) -> None:
        try:
            if self.handle:
                _lib.lib().jh_event_destroy(self.handle)
                self.handle = None
        except Exception:
            pass


def f32(x, device) -> torch.Tensor:
    """Host array -> contiguous fp32 device tensor."""
    return torch.as_tensor(np.ascontiguousarray(x, dtype=np.float32)).to(device, non_blocking=False)


class GpuModel:
    """Model constants of one task on one GPU (the counterpart of the per-thread MjModel copies,
    judo/utils/mj_rollout_backend.py:38-43 -- here a single read-only image shared by every lane)."""

    def __init__(self, task: str | dict, device: torch.device | None = None) -> None:
        self.desc = load_description(task) if isinstance(task, str) else task
        self.task = self.desc["task"]
        lay = layout(self.desc)
        self.nq, self.nv, self.nu, self.ns = lay.nq, lay.nv, lay.nu, lay.ns
        self.nx = self.nq + self.nv
        self.dt = float(self.desc["option"]["timestep"])
        self.device = device if device is not None else require_gpu()
        blob = pack_model(self.desc)
        self._blob = blob
        handle = C.c_void_p()
        buf = C.create_string_buffer(blob, len(blob))
        st = _lib.lib().jh_model_create(buf, len(blob), self.device.index or 0, C.byref(handle))
        _lib.check(st, "jh_model_create")
        self.handle = handle
        self._max_knots_cache: dict[int, int] = {}
        self.kernel_generation = 3 if self.desc.get("family", self.task) in ("leap_cube", "fr3_pick") else 2  # library defaults (jh_model_create)
        self._self_collision_requested = True
        gen = os.environ.get("JUDO_AMD_FR3_KERNEL")  # diagnostic: run the fr3_pick tests / benches on another kernel generation of the library
        if gen and self.task == "fr3_pick":
            self.set_kernel(int(gen))
        self.self_collision = self.desc.get("family", self.task) == "leap_cube"  # library default: on where the kernel models it
        # contacts a rollout can hold.  The leap kernel exists in two builds (48, all in LDS; 64 with 16 in global memory, 2.8 % slower): the headline model drops 2e-6
        # contacts per rollout-step at 48, the SHIPPED workloads of the caged / primitive-hand variants 2e-4 .. 4e-4 (tools/diag/shipped_config_stats.py): those take 64
        self.closed_form = self.task in ("cartpole", "cylinder_push")  # jh_simple.hip: rollout kernels of ~50 us -- the plan step runs as one launch that reads its host block in place
        self.contact_capacity = 0
        # caltech_leap_cube's fingertips as the kernel collides them: "sphere" (the stand-in of engine_model.kernel_stand_ins) or "cylinder" (the MJCF's geometry: an image
        # that keeps the cylinders, and with it the cylinder build of the leap kernel, 64 contacts).  The library decides from the image; this reports what it chose.
        self.fingertips = "cylinder" if self.build()["cylinder_build"] else "sphere"
        # fr3_pick: the arm's own pairs (link against link, gripper against link) are in the image or not ("self_collision" in the description); the library selects the
        # self-collision build of the fr3 kernel from the image, and this reports what it chose
        self.arm_self_collision = self.fr3_build()["self_collision_build"]
        if self.desc.get("family", self.task) == "leap_cube":
            self.set_contact_capacity(48 if self.task == "leap_cube" else 64)

    def set_kernel(self, generation: int) -> None:
        """Select the articulated-engine kernel generation (3 = cooperative, two waves per SIMD: the default; 2 = cooperative, one wave per SIMD; 1 = one lane per rollout)."""
        _lib.check(_lib.lib().jh_model_set_kernel(self.handle, int(generation)), "jh_model_set_kernel")
        self._max_knots_cache.clear()
        self.kernel_generation = int(generation)
        # only generation 3 of the leap family models the hand's own contacts: what bench.py / tests report must follow the kernel actually selected
        self.self_collision = self._self_collision_requested and self.kernel_generation == 3 and self.desc.get("family", self.task) == "leap_cube"

    def build(self) -> dict:
        """`jh_model_build`: which build of its kernel this model runs."""
        out = (C.c_int * 4)()
        _lib.check(_lib.lib().jh_model_build(self.handle, out), "jh_model_build")
        return {"kernel_generation": int(out[0]), "contact_capacity": int(out[1]), "cylinder_build": bool(out[2]), "cylinders": int(out[3])}

    def fr3_build(self) -> dict:
        """`jh_model_fr3_build`: whether this model runs the self-collision build of the fr3 kernel, and how many pairs of its image only that build collides."""
        out = (C.c_int * 4)()
        _lib.check(_lib.lib().jh_model_fr3_build(self.handle, out), "jh_model_fr3_build")
        return {"self_collision_build": bool(out[0]), "arm_pairs": int(out[1]), "default_build_accepts": bool(out[2]), "self_collision_build_accepts": bool(out[3])}

    def set_contact_capacity(self, contacts: int) -> None:
        """leap_cube family: 48 or 64 contacts per rollout (`jh_model_set_contact_capacity`)."""
        _lib.check(_lib.lib().jh_model_set_contact_capacity(self.handle, int(contacts)), "jh_model_set_contact_capacity")
        self._max_knots_cache.clear()
        self.contact_capacity = int(contacts)

    def set_self_collision(self, on: bool) -> None:
        """leap_cube, kernel generation 3: model the hand's own contacts too (default) or the cube's alone."""
        _lib.check(_lib.lib().jh_model_set_self_collision(self.handle, int(bool(on))), "jh_model_set_self_collision")
        self._self_collision_requested = bool(on)
        self.self_collision = bool(on) and self.kernel_generation == 3 and self.desc.get("family", self.task) == "leap_cube"

    def trace_layout(self) -> tuple[int, int, bool]:
        """(first sensor address, number of floats, buffer is column-major) of the trace sensors the fused kernel can write for every rollout
        (`jh_model_trace_layout`); 0 floats: none."""
        out = (C.c_int * 3)()
        _lib.check(_lib.lib().jh_model_trace_layout(self.handle, out), "jh_model_trace_layout")
        return int(out[0]), int(out[1]), bool(out[2])

    def limits(self) -> tuple[int, int, int, int]:
        """`jh_model_limits`: (largest fused knot count, JH_MAX_KNOT_DIM, JH_MAX_ELITES, contact capacity per rollout)."""
        out = (C.c_int * 4)()
        _lib.check(_lib.lib().jh_model_limits(self.handle, out), "jh_model_limits")
        return tuple(int(v) for v in out)

    @property
    def max_fused_knots(self) -> int:
        """Largest knot count the fused rollout kernel of this model accepts (`jh_model_limits`)."""
        out = (C.c_int * 4)()
        _lib.check(_lib.lib().jh_model_limits(self.handle, out), "jh_model_limits")
        return int(out[0])

    def max_fused_knots_at(self, H: int) -> int:
        """Largest K `jh_rollout_cost` accepts for a launch of H steps (the one-lane kernels stage W and the knots in LDS: it depends on H)."""
        H = int(H)
        k = self._max_knots_cache.get(H)  # (asked once per plan step; the answer changes with the kernel generation / contact capacity only: those setters clear the cache)
        if k is None:
            k = int(_lib.lib().jh_model_max_fused_knots(self.handle, H))
            if k < 0:
                _lib.check(k, "jh_model_max_fused_knots")
            self._max_knots_cache[H] = k
        return k

    def one_launch_max_knots_at(self, H: int) -> int:
        """Largest K whose plan step runs as one launch at horizon H (`jh_model_one_launch_max_knots`; 0: the model has no one-launch form)."""
        k = int(_lib.lib().jh_model_one_launch_max_knots(self.handle, int(H)))
        if k < 0:
            _lib.check(k, "jh_model_one_launch_max_knots")
        return k

    def set_plan_step_launches(self, launches: int) -> None:
        """0: one launch where it fits (default), 1: always one launch, 2: always two (`jh_model_set_plan_step_launches`)."""
        _lib.check(_lib.lib().jh_model_set_plan_step_launches(self.handle, int(launches)), "jh_model_set_plan_step_launches")

    def set_rollout_schedule(self, mode: int) -> None:
        """leap_cube, kernel generation 3: 0 = persistent waves on a queue of rollout groups where the launch exceeds the GPU's wave slots (default), 1 = always the static
        grid, 2 = the queue wherever the kernel has it (`jh_model_set_rollout_schedule`).  The bits do not depend on it."""
        _lib.check(_lib.lib().jh_model_set_rollout_schedule(self.handle, int(mode)), "jh_model_set_rollout_schedule")

    def set_rollout_slices(self, slices: int = 0, max_workgroups: int = 0, flags: int = 0) -> None:
        """leap_cube, kernel generation 3, the queue's units: `slices` 0 = (group, horizon slice) where the queue runs and the launch has at least two groups per resident
        wave (default), 1..64 = that many slices wherever the queue runs (1: whole groups).  `max_workgroups` > 0 caps the queue's grid and `flags` bit 0 makes every
        hand-off count as missed: test hooks (`jh_model_set_rollout_slices`).  The bits do not depend on any of it."""
        _lib.check(_lib.lib().jh_model_set_rollout_slices(self.handle, int(slices), int(max_workgroups), int(flags)), "jh_model_set_rollout_slices")

    def last_rollout_slices(self) -> int:
        """What the last fused launch ran: 0 = the static grid, 1 = the queue of whole groups, S > 1 = the queue of S slices per group."""
        return int(_lib.lib().jh_model_last_rollout_slices(self.handle))

    def set_rollout_slice_bounds(self, first_steps=()) -> None:
        """leap_cube, kernel generation 3: an explicit schedule of the queue's slices -- the first steps of slices 1 .. n, positive and strictly increasing, at most 15; empty
        clears it.  Entries at or behind a launch's horizon are dropped at that launch.  Of this and `set_rollout_slices` the later call decides the slices
        (`jh_model_set_rollout_slice_bounds`).  The bits do not depend on it."""
        steps = [int(s) for s in first_steps]
        arr = (C.c_int * max(1, len(steps)))(*steps)
        _lib.check(_lib.lib().jh_model_set_rollout_slice_bounds(self.handle, arr, len(steps)), "jh_model_set_rollout_slice_bounds")

    def last_rollout_slice_bounds(self) -> tuple:
        """The first steps of slices 1 .. S - 1 of the last fused launch (empty: whole groups, or the static grid)."""
        out = (C.c_int * 63)()
        n = int(_lib.lib().jh_model_last_rollout_slice_bounds(self.handle, out, 63))
        if n < 0:
            _lib.check(n, "jh_model_last_rollout_slice_bounds")
        return tuple(out[:n])

    def recomputed_units(self) -> int:
        """Queue units that missed their hand-off and recomputed their group up to their slice, since the counters were last reset by `stats()` (synchronises)."""
        v = int(_lib.lib().jh_model_recomputed_units(self.handle))
        if v < 0:
            _lib.check(v, "jh_model_recomputed_units")
        return v

    def stats(self, reset: bool = True) -> dict:
        """Diagnostic counters of the articulated-body kernels (synchronises)."""
        out = (C.c_int * 8)()
        _lib.check(_lib.lib().jh_model_stats(self.handle, out, int(reset)), "jh_model_stats")
        u = [v & 0xFFFFFFFF for v in out]  # 32-bit counters: unsigned
        return {"contact_overflow": u[0], "newton_cap_hits": u[1], "newton_iters": u[2], "steps": u[3], "wave_newton_iters": u[4], "wave_steps": u[5], "overflow_pool_fallbacks": u[6], "one_launch_plan_steps": u[7]}

    def __del__(self) -> None:
        try:
            if getattr(self, "handle", None):
                _lib.lib().jh_model_destroy(self.handle)
                self.handle = None
        except Exception:
            pass


class GpuModelSet:
    """B `GpuModel`s whose images differ in the float section alone, as ONE device buffer for `jh_plan_step_batch_models` (include/judo_amd.h): problem b of the batched
    plan step runs on `models[b]`'s constants.  The library checks the members (same dimensions, int section, kernel build and settings; each image acceptable to its
    kernel) and raises ValueError / JudoAmdError naming the member and the field.  The set keeps its members alive: member 0's handle stays in use for everything but the
    float sections, and its `stats()` collect the counters of the whole launch.  fr3_pick members make an fr3 set (`jh_fr3_model_set_create`, `fr3` is True), which the
    entries that carry a phase plan: `jh_plan_step_batch_phases_models` and `jh_plan_step_randomized_phase`."""

    def __init__(self, models) -> None:
        self.models = list(models)
        if not self.models:
            raise ValueError("a model set needs at least one model")
        handles = (C.c_void_p * len(self.models))(*[m.handle.value for m in self.models])
        handle = C.c_void_p()
        # the members' family picks the constructor: fr3_pick members alone make an fr3 set, which the phase-taking entries plan (`jh_plan_step_batch_phases_models`,
        # `jh_plan_step_randomized_phase`); anything else, a mixture included, goes to the generic constructor and meets its checks
        self.fr3 = all(m.desc.get("family", m.task) == "fr3_pick" for m in self.models)
        create = "jh_fr3_model_set_create" if self.fr3 else "jh_model_set_create"
        _lib.check(getattr(_lib.lib(), create)(handles, len(self.models), C.byref(handle)), create)
        self.handle = handle

    def __len__(self) -> int:
        return len(self.models)

    def info(self) -> dict:
        """`jh_model_set_info`: members, floats per image, floats from one image to the next, members whose image differs from member 0's."""
        out = (C.c_int * 4)()
        _lib.check(_lib.lib().jh_model_set_info(self.handle, out), "jh_model_set_info")
        return {"B": int(out[0]), "image_floats": int(out[1]), "stride_floats": int(out[2]), "distinct_from_first": int(out[3])}

    def pair_tables(self) -> bool:
        """`jh_model_set_pair_tables`: do the set's launches use the hand's pair tables (every member agrees with member 0 on what they were computed from)?"""
        return bool(_lib.lib().jh_model_set_pair_tables(self.handle))

    def update(self, b: int, model: GpuModel) -> None:
        """Replace member b's image (`jh_model_set_update`: the same checks; synchronous -- between episodes, not in the plan loop)."""
        _lib.check(_lib.lib().jh_model_set_update(self.handle, int(b), model.handle), "jh_model_set_update")
        self.models[int(b)] = model

    def close(self) -> None:
        if getattr(self, "handle", None):
            _lib.lib().jh_model_set_destroy(self.handle)
            self.handle = None

    def __del__(self) -> None:
        try:
            self.close()
        except Exception:
            pass


def rollout_slice_schedule(horizon: int, groups: int, wave_slots: int) -> tuple:
    """The leap queue's automatic schedule of horizon slices as a pure function of the launch's shape (`jh_rollout_slice_schedule`; no device needed): the first steps of
    slices 1 .. n for `groups` groups of four rollouts over `horizon` steps on a GPU that holds `wave_slots` waves of the kernel.  Empty: whole groups."""
    out = (C.c_int * 15)()
    n = int(_lib.lib().jh_rollout_slice_schedule(int(horizon), int(groups), int(wave_slots), out, 15))
    if n < 0:
        _lib.check(n, "jh_rollout_slice_schedule")
    return tuple(out[:n])
