#!/usr/bin/env python3
"""Golden vectors for the spot_box_push task layer (runs ONLY in the build container, needs the reference checkout tools/_ref_import.py points at).

Recorded from the reference's own numpy code, imported through tools/_ref_import.py with a namespace object standing in for `self` (constructing the real task needs
MuJoCo, which this image lacks), as tools/gen_golden_spot.py does for the other Spot tasks:

  B1  SpotBoxPush.reward                          judo/tasks/spot/spot_box_push.py:63-115   (default config, and one with every weight changed)
  B2  SpotBoxPushConfig defaults                  judo/tasks/spot/spot_box_push.py:25-45
  B3  override-resolved optimizer / controller configs for spot_box_push   judo/optimizers/overrides.py, judo/controller/overrides.py

Index facts the reward reads (`get_joint_position_start_index` / `get_sensor_start_index` of judo/models/xml/spot_box/robot.xml): base qpos at 0, box_joint qpos
at 26, object_y_axis at sensor float 9, trace_fngr_site at 15; nq = 33.
"""

from __future__ import annotations

import json
import os
import sys
from types import SimpleNamespace

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _ref_import  # noqa: E402

_ref_import.install()

from judo.controller.controller import ControllerConfig  # noqa: E402
from judo.optimizers.cem import CrossEntropyMethodConfig  # noqa: E402
from judo.optimizers.mppi import MPPIConfig  # noqa: E402
from judo.optimizers.ps import PredictiveSamplingConfig  # noqa: E402
from judo.tasks.spot.spot_box_push import SpotBoxPush, SpotBoxPushConfig  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden")
NQ, NV, NS = 33, 31, 39


def _rollouts(rng, N, T):
    """States / sensors in the spot_box layout: some rollouts fall (base height at and below the 0.35 threshold), some turn the box's y axis up (> 0.5, at 0.5 exactly)."""
    states = rng.standard_normal((N, T, NQ + NV)) * 0.5
    states[:, :, 2] = 0.5 + rng.standard_normal((N, T)) * 0.05
    states[1, 3, 2] = 0.35      # exactly at the fallen threshold (<=)
    states[2, :, 2] = 0.2       # fallen throughout
    states[:, :, 26:29] = rng.uniform(-2, 2, (N, T, 3))
    sensors = rng.standard_normal((N, T, NS)) * 0.3
    y = rng.standard_normal((N, T, 3))
    y /= np.linalg.norm(y, axis=-1, keepdims=True)
    y[3, :, :] = [0.0, 0.0, 1.0]          # box on its side: y axis up in every step
    y[4, ::2, :] = [0.0, 0.6, 0.8]        # every other step
    y[5, 1, :] = [0.0, np.sqrt(0.75), 0.5]  # exactly at the orientation threshold (> is strict)
    sensors[:, :, 9:12] = y
    return states, sensors


def main() -> None:
    rng = np.random.default_rng(7)
    out: dict[str, np.ndarray] = {}
    N, T, nu = 8, 11, 10
    states, sensors = _rollouts(rng, N, T)
    controls = rng.standard_normal((N, T, nu))
    out["states"], out["sensors"], out["controls"] = states, sensors, controls
    cfg = SpotBoxPushConfig()
    s = SimpleNamespace(config=cfg, model=SimpleNamespace(nq=NQ), body_pose_idx=0, object_pose_idx=26, object_y_axis_idx=9, gripper_pos_idx=15)
    out["reward"] = SpotBoxPush.reward(s, states, sensors, controls)
    cfg2 = SpotBoxPushConfig()
    cfg2.goal_position = np.array([1.0, -0.5, 0.254])
    cfg2.w_goal, cfg2.w_orientation, cfg2.w_torso_proximity, cfg2.w_gripper_proximity = 30.0, 5.0, 0.7, 2.0
    cfg2.orientation_threshold, cfg2.fall_penalty, cfg2.w_controls, cfg2.spot_fallen_threshold = 0.3, 1000.0, 0.2, 0.4
    s.config = cfg2
    out["reward_cfg2"] = SpotBoxPush.reward(s, states, sensors, controls)
    out["cfg2"] = np.array([*cfg2.goal_position, cfg2.w_goal, cfg2.w_orientation, cfg2.w_torso_proximity, cfg2.w_gripper_proximity, cfg2.orientation_threshold,
                            cfg2.fall_penalty, cfg2.w_controls, cfg2.spot_fallen_threshold])
    np.savez_compressed(os.path.join(OUT, "spot_box_push.npz"), **out)
    res: dict = {"optimizer": {}, "controller": {}}
    for name, cfg_cls in (("mppi", MPPIConfig), ("cem", CrossEntropyMethodConfig), ("ps", PredictiveSamplingConfig)):
        c = cfg_cls()
        c.set_override("spot_box_push")
        res["optimizer"][name] = dict(vars(c))
    c = ControllerConfig()
    c.set_override("spot_box_push")
    res["controller"] = dict(vars(c))
    res["task_defaults"] = vars(SpotBoxPushConfig())
    with open(os.path.join(OUT, "spot_box_push_configs.json"), "w") as f:
        json.dump(res, f, indent=1, default=lambda o: o.tolist() if hasattr(o, "tolist") else str(o))
    for fn in ("spot_box_push.npz", "spot_box_push_configs.json"):
        print(fn, os.path.getsize(os.path.join(OUT, fn)))


if __name__ == "__main__":
    main()
