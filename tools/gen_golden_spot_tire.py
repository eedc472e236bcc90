#!/usr/bin/env python3
"""Golden vectors for the spot_tire_roll / spot_tire_upright task layer (runs ONLY in the build container, needs the reference checkout tools/_ref_import.py points at).

Recorded from the reference's own numpy code, imported through tools/_ref_import.py with a namespace object standing in for `self` (constructing the real task needs
MuJoCo, which this image lacks), as tools/gen_golden_spot_box.py does for spot_box_push:

  T1  SpotTireRoll.reward                 judo/tasks/spot/spot_tire_roll.py:73-137      (default config, and one with every weight changed)
  T2  SpotTireUpright.reward              judo/tasks/spot/spot_tire_upright.py:99-235   (default config, and one with every weight changed)
  T3  the use_legs=True, use_gripper=False command layout of spot_tire_upright: actuator_ctrlrange, task_to_sim_ctrl (1-D, 2-D, 3-D controls, every leg-selection
      band), get_action_components                                     judo/tasks/spot/spot_base.py:166-461
  T4  both configs' defaults and the override-resolved optimizer / controller configs            judo/optimizers/overrides.py, judo/controller/overrides.py

Index facts the rewards read (`get_joint_position_start_index` / `get_sensor_start_index` / jnt_dofadr of judo/models/xml/spot_tire/robot.xml): base qpos at 0,
tire_joint qpos at 26 and dof at 25, object_y_axis at sensor float 9, trace_fngr_site at 15, fl_pos at 27, fr_pos at 30; nq = 33.
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
from judo.tasks.spot import spot_constants as SC  # noqa: E402
from judo.tasks.spot.spot_base import SpotBase  # noqa: E402
from judo.tasks.spot.spot_tire_roll import SpotTireRoll, SpotTireRollConfig  # noqa: E402
from judo.tasks.spot.spot_tire_upright import SpotTireUpright, SpotTireUprightConfig  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden")
NQ, NV, NS = 33, 31, 60


def _rollouts(rng, N, T):
    """States / sensors in the spot_tire layout: falls (base height at and below 0.35), a tire leaning past 0.1 (and exactly at it), grippers near and inside the tire."""
    states = rng.standard_normal((N, T, NQ + NV)) * 0.5
    states[:, :, 2] = 0.5 + rng.standard_normal((N, T)) * 0.05
    states[1, 3, 2] = 0.35      # exactly at the fallen threshold (<=)
    states[2, :, 2] = 0.2       # fallen throughout
    states[:, :, 26:29] = rng.uniform(-2, 2, (N, T, 3))
    states[:, :, 28] = np.abs(states[:, :, 28]) * 0.2
    sensors = rng.standard_normal((N, T, NS)) * 0.3
    y = rng.standard_normal((N, T, 3))
    y /= np.linalg.norm(y, axis=-1, keepdims=True)
    y[3, :, :] = [0.0, 1.0, 0.0]              # upright throughout
    y[4, ::2, :] = [0.0, 0.6, 0.8]            # leaning every other step
    y[5, 1, :] = [0.0, np.sqrt(0.99), 0.1]    # exactly at the tire-fallen threshold (> is strict)
    sensors[:, :, 9:12] = y
    sensors[6, :, 15:18] = states[6, :, 26:29] + 0.05   # gripper inside the tire's half radius
    sensors[7, :, 15:18] = states[7, :, 26:29] + [0.5, 0.0, 0.0]
    sensors[7, :, 17] = 0.1                            # far from the centre and below 2 half widths + 0.05
    return states, sensors


def _legs_self():
    s = SimpleNamespace(use_arm=True, use_gripper=False, use_legs=True, use_torso=False, leg_selection_index=None, gripper_selection_index=None)
    SpotBase.set_command_values(s)
    s.default_policy_command = np.array([0, 0, 0] + list(SC.ARM_STOWED_POS) + [0] * 12 + [0, 0, SC.STANDING_HEIGHT_CMD])
    s.apply_selection_mask = lambda c: SpotBase.apply_selection_mask(s, c)
    return s


def main() -> None:
    rng = np.random.default_rng(11)
    out: dict[str, np.ndarray] = {}
    N, T = 8, 11
    states, sensors = _rollouts(rng, N, T)
    out["states"], out["sensors"] = states, sensors
    # T1
    c_roll = rng.standard_normal((N, T, 11))
    out["controls_roll"] = c_roll
    s = SimpleNamespace(config=SpotTireRollConfig(), model=SimpleNamespace(nq=NQ), body_pose_idx=0, object_pose_idx=26, gripper_pos_idx=15, object_y_axis_idx=9,
                        object_vel_idx=25)
    out["reward_roll"] = SpotTireRoll.reward(s, states, sensors, c_roll)
    cfg = SpotTireRollConfig()
    cfg.goal_position = np.array([1.0, -0.5, 0.33])
    cfg.fall_penalty, cfg.tire_fallen_threshold, cfg.w_goal, cfg.w_torso_proximity, cfg.torso_goal_offset = 3000.0, 0.2, 30.0, 2.0, 0.8
    cfg.w_gripper_proximity, cfg.gripper_goal_offset, cfg.gripper_goal_altitude, cfg.w_tire_linear_velocity = 1.5, 0.2, 0.1, 5.0
    cfg.w_tire_angular_velocity, cfg.w_controls, cfg.spot_fallen_threshold = 0.5, 0.3, 0.4
    s.config = cfg
    out["reward_roll_cfg2"] = SpotTireRoll.reward(s, states, sensors, c_roll)
    out["cfg2_roll"] = np.array([*cfg.goal_position, cfg.fall_penalty, cfg.tire_fallen_threshold, cfg.w_goal, cfg.w_torso_proximity, cfg.torso_goal_offset,
                                 cfg.w_gripper_proximity, cfg.gripper_goal_offset, cfg.gripper_goal_altitude, cfg.w_tire_linear_velocity, cfg.w_tire_angular_velocity,
                                 cfg.w_controls, cfg.spot_fallen_threshold])
    # T2
    c_up = rng.standard_normal((N, T, 17))
    out["controls_upright"] = c_up
    s = SimpleNamespace(config=SpotTireUprightConfig(), model=SimpleNamespace(nq=NQ), body_pose_idx=0, object_pose_idx=26, tire_y_axis_idx=9, gripper_pos_idx=15,
                        fl_pos_idx=27, fr_pos_idx=30)
    out["reward_upright"] = SpotTireUpright.reward(s, states, sensors, c_up)
    cfg = SpotTireUprightConfig()
    cfg.orientation_error_smoothing_width, cfg.w_tire_orientation, cfg.w_gripper_proximity, cfg.w_foot_proximity = 0.5, 100.0, 4.0, 7.0
    cfg.w_torso_proximity, cfg.gripper_too_inside_tire_penalty, cfg.gripper_not_above_tire_penalty, cfg.w_controls = 2.0, 50.0, 70.0, 0.5
    cfg.fall_penalty, cfg.spot_fallen_threshold = 4000.0, 0.4
    s.config = cfg
    out["reward_upright_cfg2"] = SpotTireUpright.reward(s, states, sensors, c_up)
    out["cfg2_upright"] = np.array([cfg.orientation_error_smoothing_width, cfg.w_tire_orientation, cfg.w_gripper_proximity, cfg.w_foot_proximity, cfg.w_torso_proximity,
                                    cfg.gripper_too_inside_tire_penalty, cfg.gripper_not_above_tire_penalty, cfg.w_controls, cfg.fall_penalty, cfg.spot_fallen_threshold])
    # T3
    s = _legs_self()
    nu = len(s.default_command)
    out["legs_ctrlrange"] = SpotBase.actuator_ctrlrange.fget(s)
    ctl = rng.uniform(-1, 1, (6, 5, nu))
    ctl[:, :, s.leg_selection_index] = np.array([-0.9, -0.5, 0.0, 0.5, 0.51, 0.9])[:, None]
    out["legs_controls"] = ctl
    out["legs_sim3"] = SpotBase.task_to_sim_ctrl(s, ctl)
    out["legs_sim2"] = SpotBase.task_to_sim_ctrl(s, ctl[:, 0])
    out["legs_sim1"] = SpotBase.task_to_sim_ctrl(s, ctl[0, 0])
    np.savez_compressed(os.path.join(OUT, "spot_tire.npz"), **out)
    res: dict = {"legs_action_components": SpotBase.get_action_components(s)}
    for task, cfg_cls in (("spot_tire_roll", SpotTireRollConfig), ("spot_tire_upright", SpotTireUprightConfig)):
        r: dict = {"optimizer": {}, "controller": {}}
        for name, ocls in (("mppi", MPPIConfig), ("cem", CrossEntropyMethodConfig), ("ps", PredictiveSamplingConfig)):
            c = ocls()
            c.set_override(task)
            r["optimizer"][name] = dict(vars(c))
        c = ControllerConfig()
        c.set_override(task)
        r["controller"] = dict(vars(c))
        r["task_defaults"] = vars(cfg_cls())
        res[task] = r
    with open(os.path.join(OUT, "spot_tire_configs.json"), "w") as f:
        json.dump(res, f, indent=1, default=lambda o: o.tolist() if hasattr(o, "tolist") else str(o))
    for fn in ("spot_tire.npz", "spot_tire_configs.json"):
        print(fn, os.path.getsize(os.path.join(OUT, fn)))


if __name__ == "__main__":
    main()
