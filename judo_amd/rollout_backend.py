"""RolloutBackend on the GPU -- the drop-in seam (judo/utils/rollout_backend.py:10-46).

`GpuRolloutBackend.rollout(x0, controls, last_policy_output=None) -> (states, sensors, None)` has the contract of
`MJRolloutBackend.rollout` (judo/utils/mj_rollout_backend.py:45-88): x0 (nq+nv,) is tiled over the batch (or given
per rollout), controls are (num_threads, T, nu); states[n,t] is the state after applying controls[n,t]; sensors[n,t] is
the sensordata of the step that produced it.  One lane per rollout replaces one OS thread + one MjModel copy per rollout;
`update(num_threads)` therefore only records the new batch size.

`rollout_plants(model_set, plant_of_block, x0, controls)` is the same call on the plants of a `GpuModelSet` -- a plant per block of rollouts, one launch
(`jh_rollout_materialize_plants`): what a judo-side controller calls for an ensemble of plants or for domain randomisation.
"""

from __future__ import annotations

import ctypes as C
from abc import ABC, abstractmethod

import numpy as np
import torch

from judo_amd import _lib
from judo_amd.device import GpuModel, GpuModelSet, current_stream_ptr, f32


class RolloutBackend(ABC):
    num_threads: int

    @abstractmethod
    def rollout(self, x0: np.ndarray, controls: np.ndarray, last_policy_output: np.ndarray | None = None):
        ...

    @abstractmethod
    def update(self, num_threads: int) -> None:
        ...


class GpuRolloutBackend(RolloutBackend):
    def __init__(self, model: GpuModel | str, num_threads: int) -> None:
        self.model = model if isinstance(model, GpuModel) else GpuModel(model)
        self.num_threads = int(num_threads)

    def rollout_device(self, x0: torch.Tensor, controls: torch.Tensor, want_states: bool = True, want_sensors: bool = True):
        """Device tensors in, device tensors out (fp32)."""
        gm = self.model
        if controls.ndim != 3:
            raise ValueError(f"controls must be (num_threads, T, nu), got {tuple(controls.shape)}")
        N, H, nu = (int(s) for s in controls.shape)
        if nu != gm.nu:
            raise ValueError(f"controls.shape[-1] = {nu} != nu = {gm.nu}")
        batched = int(x0.ndim == 2)
        if x0.shape[-1] != gm.nx:
            raise ValueError(f"x0 must have {gm.nx} = nq+nv entries, got {tuple(x0.shape)}")
        if batched and x0.shape[0] != N:
            raise ValueError(f"batched x0 has {x0.shape[0]} rows but controls has {N}")
        if not want_states and not want_sensors:
            raise ValueError("nothing to compute: both outputs disabled")
        x0 = x0.to(torch.float32).contiguous()
        controls = controls.to(torch.float32).contiguous()
        states = torch.empty((N, H, gm.nx), dtype=torch.float32, device=gm.device) if want_states else None
        sensors = torch.empty((N, H, gm.ns), dtype=torch.float32, device=gm.device) if want_sensors else None
        st = _lib.lib().jh_rollout_materialize(gm.handle, _lib.ptr(x0), batched, _lib.ptr(controls), N, H, _lib.ptr(states), _lib.ptr(sensors), current_stream_ptr())
        _lib.check(st, "jh_rollout_materialize")
        return states, sensors

    def rollout(self, x0: np.ndarray, controls: np.ndarray, last_policy_output: np.ndarray | None = None):
        x0 = np.asarray(x0)
        controls = np.asarray(controls)
        if controls.ndim != 3 or controls.shape[0] != (x0.shape[0] if x0.ndim == 2 else controls.shape[0]):
            raise ValueError("controls must be (num_threads, T, nu) with one row per rollout")
        states, sensors = self.rollout_device(f32(x0, self.model.device), f32(controls, self.model.device))
        return states.cpu().numpy().astype(np.float64), sensors.cpu().numpy().astype(np.float64), None

    def rollout_plants_device(self, model_set: GpuModelSet, plant_of_block, x0: torch.Tensor, controls: torch.Tensor, shared_controls: bool = False,
                              want_states: bool = True, want_sensors: bool = True):
        """`rollout_device` on the plants of a `GpuModelSet` (`jh_rollout_materialize_plants`, or `jh_fr3_rollout_materialize_plants` for an fr3_pick set; one launch): G = len(plant_of_block) blocks of n rollouts, block g -- rows
        [g * n, (g + 1) * n) of the outputs -- on plant `plant_of_block[g]`.  controls are (G * n, T, nu), or with `shared_controls` (n, T, nu), which every block rolls
        out; x0 is (nq+nv,) or (G * n, nq+nv).  A block's rows are bit for bit `rollout_device` on that plant's own model."""
        table = check_plant_table(plant_of_block, len(model_set))
        gm, G = model_set.models[0], len(table)
        if controls.ndim != 3:
            raise ValueError(f"controls must be ({'n' if shared_controls else 'G * n'}, T, nu), got {tuple(controls.shape)}")
        rows, H, nu = (int(s) for s in controls.shape)
        if nu != gm.nu:
            raise ValueError(f"controls.shape[-1] = {nu} != nu = {gm.nu}")
        if not shared_controls and rows % G != 0:
            raise ValueError(f"controls has {rows} rows, which do not split into G = {G} equal blocks")
        n = rows if shared_controls else rows // G
        batched = int(x0.ndim == 2)
        if x0.shape[-1] != gm.nx:
            raise ValueError(f"x0 must have {gm.nx} = nq+nv entries, got {tuple(x0.shape)}")
        if batched and x0.shape[0] != G * n:
            raise ValueError(f"batched x0 has {x0.shape[0]} rows but the launch has G * n = {G * n}")
        if not want_states and not want_sensors:
            raise ValueError("nothing to compute: both outputs disabled")
        x0 = x0.to(torch.float32).contiguous()
        controls = controls.to(torch.float32).contiguous()
        states = torch.empty((G * n, H, gm.nx), dtype=torch.float32, device=gm.device) if want_states else None
        sensors = torch.empty((G * n, H, gm.ns), dtype=torch.float32, device=gm.device) if want_sensors else None
        # (an fr3_pick set has an entry of its own, as every fr3 form has: the cooperative arm kernel's launch on plants)
        entry = "jh_fr3_rollout_materialize_plants" if getattr(model_set, "fr3", False) else "jh_rollout_materialize_plants"
        st = getattr(_lib.lib(), entry)(model_set.handle, (C.c_int * G)(*table), G, n, _lib.ptr(x0), batched, _lib.ptr(controls), int(bool(shared_controls)), H,
                                        _lib.ptr(states), _lib.ptr(sensors), current_stream_ptr())
        _lib.check(st, entry)
        return states, sensors

    def rollout_plants(self, model_set: GpuModelSet, plant_of_block, x0: np.ndarray, controls: np.ndarray, last_policy_output: np.ndarray | None = None,
                       shared_controls: bool = False):
        """`rollout` with a plant per rollout block: the reference's signature behind the set and the table (`rollout_plants_device`)."""
        x0 = np.asarray(x0)
        controls = np.asarray(controls)
        dev = model_set.models[0].device
        states, sensors = self.rollout_plants_device(model_set, plant_of_block, f32(x0, dev), f32(controls, dev), shared_controls=shared_controls)
        return states.cpu().numpy().astype(np.float64), sensors.cpu().numpy().astype(np.float64), None

    def update(self, num_threads: int) -> None:
        self.num_threads = int(num_threads)


def check_plant_table(plant_of_block, members: int) -> list[int]:
    """`plant_of_block` as a list of G plant indices, 1 <= G <= MAX_FLEET_PLANT_BLOCKS, each in [0, members); raises ValueError naming the block.  No device needed."""
    raw = list(plant_of_block)
    if not 1 <= len(raw) <= _lib.MAX_FLEET_PLANT_BLOCKS:
        raise ValueError(f"a table of {len(raw)} blocks is outside [1, {_lib.MAX_FLEET_PLANT_BLOCKS}] (include/judo_amd.h JH_MAX_FLEET_PLANT_BLOCKS)")
    table = []
    for g, p in enumerate(raw):
        if isinstance(p, bool) or int(p) != p or not 0 <= int(p) < members:
            raise ValueError(f"plant_of_block[{g}] = {p!r} outside [0, M = {members}): block {g} names no plant of the set")
        table.append(int(p))
    return table
