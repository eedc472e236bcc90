"""Spot tasks on the policy rollout (judo/tasks/spot/spot_base.py, spot_navigate.py, spot_constants.py).

A Spot task optimises a compact command vector (base velocity, optionally arm / front-leg / torso targets), `task_to_sim_ctrl` expands it
to the 25-d command of the locomotion policy, and the rollout runs policy + plant (`judo_amd.policy.PolicyRolloutBackend`).  Everything
here accepts numpy arrays (host, float64, what the reference passes) or torch tensors (device, what the controller's materialise path passes).

Scope: the robot alone on the ground plane (`spot_base`, `spot_navigate`), the robot with a free box (`spot_box_push`, model `spot_box`) and with a free tire
(`spot_tire_roll`, `spot_tire_upright`, model `spot_tire`: the tire's meshes, absent upstream, stand in as the reference's own cylinder approximation, DESIGN.md
section 8) -- the tree kernel's object instantiations, csrc/jh_engine_v4.hip.
"""

from __future__ import annotations

from dataclasses import dataclass, field
from typing import Any

import numpy as np

from judo_amd.tasks import Task, TaskConfig, register_task

# ---- judo/tasks/spot/spot_constants.py -------------------------------------------------------------------------------
DEFAULT_SPOT_ROLLOUT_CUTOFF_TIME = 0.125   # :18
POLICY_OUTPUT_DIM = 12                     # :23
GRIPPER_CLOSED_POS, GRIPPER_OPEN_POS = 0.0, -1.54   # :52-53
LEGS_STANDING_POS = np.array([0.12, 0.72, -1.45, -0.12, 0.72, -1.45, 0.12, 0.72, -1.45, -0.12, 0.72, -1.45])   # :55-70
LEGS_STANDING_POS_RL = np.array([0.12, 0.5, -1.0, -0.12, 0.5, -1.0, 0.12, 0.5, -1.0, -0.12, 0.5, -1.0])        # :73-88
ARM_STOWED_POS = np.array([0, -3.11, 3.13, 1.56, 0, -1.56, GRIPPER_CLOSED_POS])     # :90
ARM_UNSTOWED_POS = np.array([0, -0.9, 1.8, 0, -0.9, 0, GRIPPER_CLOSED_POS])         # :92
STANDING_HEIGHT = 0.52                     # :95
STANDING_HEIGHT_CMD = STANDING_HEIGHT      # :96
Z_AXIS = np.array([0.0, 0.0, 1.0])         # :120
BOX_HALF_LENGTH = 0.254                    # :127
TIRE_RADIUS, TIRE_HALF_WIDTH = 0.33, 0.17  # :123-124
LEG_SOFT_LOWER_JOINT_LIMITS = np.array([-0.6, -0.8, -2.7] * 4)    # :99
LEG_SOFT_UPPER_JOINT_LIMITS = np.array([0.6, 1.65, -0.3] * 4)     # :100
ARM_SOFT_LOWER_JOINT_LIMITS = ARM_UNSTOWED_POS - np.array([1.0, 1.0, 0.8, np.pi / 2, 0.7, np.pi / 4, 0])   # :101
ARM_SOFT_UPPER_JOINT_LIMITS = ARM_UNSTOWED_POS + np.array([1.0, 0.8, 0.6, np.pi / 2, 0.9, np.pi / 4, 0])   # :102
BASE_VEL_CMD_INDS, ARM_CMD_INDS, FRONT_LEG_CMD_INDS, TORSO_CMD_INDS = [0, 1, 2], list(range(3, 10)), list(range(10, 16)), [22, 23, 24]   # :106-109
BASE_SOFT_LIMITS = 0.7 * np.ones(3)        # :112
TORSO_LOWER, TORSO_UPPER = np.array([-0.0, -1.0, 0.3]), np.array([+0.0, +1.0, 1.0])   # :115-116


@dataclass
class SpotBaseConfig(TaskConfig):          # spot_base.py:56-66
    fall_penalty: float = 2500.0
    spot_fallen_threshold: float = 0.35
    w_goal: float = 60.0
    w_controls: float = 0.0


def _is_torch(x) -> bool:
    return type(x).__module__.startswith("torch")


class SpotBase(Task[SpotBaseConfig]):
    """spot_base.py:72-470: the compact command vector and its mapping to the policy command; zero reward."""

    name = "spot_base"
    model_name = "spot"
    config_t = SpotBaseConfig

    def __init__(self, use_arm: bool = True, use_gripper: bool = False, use_legs: bool = False, use_torso: bool = False, config: SpotBaseConfig | None = None) -> None:
        self.use_arm, self.use_gripper, self.use_legs, self.use_torso = use_arm, use_gripper, use_legs, use_torso
        self.leg_selection_index: int | None = None
        self.gripper_selection_index: int | None = None
        self.set_command_values()
        self.default_policy_command = np.array([0, 0, 0] + list(ARM_STOWED_POS) + [0] * 12 + [0, 0, STANDING_HEIGHT_CMD])   # :159-161
        super().__init__()
        if config is not None:
            self.config = config
        self.reset()

    # ---- facts -----------------------------------------------------------------------------------------------------------
    @property
    def physics_substeps(self) -> int:     # :113-116
        return 2

    @property
    def uses_locomotion_policy(self) -> bool:
        return True

    @property
    def locomotion_policy_path(self) -> str:
        from judo_amd.policy import POLICY_PATH

        return POLICY_PATH

    @property
    def nu(self) -> int:                   # :166-169
        return len(self.default_command)

    def task_params(self, system_metadata=None) -> np.ndarray:
        return np.zeros(0, dtype=np.float32)

    def gpu_model(self, device=None):
        raise NotImplementedError("Spot tasks roll out through PolicyRolloutBackend (policy + tree kernel), not through a GpuModel")

    @property
    def actuator_ctrlrange(self) -> np.ndarray:   # :171-224
        grip_lo = GRIPPER_OPEN_POS if self.use_gripper else GRIPPER_CLOSED_POS
        arm_lo = np.concatenate((ARM_SOFT_LOWER_JOINT_LIMITS[:-1], [grip_lo]))
        arm_hi = np.concatenate((ARM_SOFT_UPPER_JOINT_LIMITS[:-1], [GRIPPER_CLOSED_POS]))
        lo, hi = [-BASE_SOFT_LIMITS], [BASE_SOFT_LIMITS]
        if self.use_arm:
            lo.append(arm_lo); hi.append(arm_hi)
            if self.use_gripper:
                lo.append(-np.ones(1)); hi.append(np.ones(1))
        if self.use_legs:
            lo += [LEG_SOFT_LOWER_JOINT_LIMITS[0:6], -np.ones(1)]; hi += [LEG_SOFT_UPPER_JOINT_LIMITS[0:6], np.ones(1)]
        if self.use_torso:
            lo.append(TORSO_LOWER); hi.append(TORSO_UPPER)
        return np.stack([np.concatenate(lo), np.concatenate(hi)], axis=-1)

    def set_command_values(self) -> None:  # :226-263
        self.leg_selection_index = self.gripper_selection_index = None
        vals: list[float] = [0, 0, 0]
        mask = list(BASE_VEL_CMD_INDS)
        if self.use_arm:
            vals += list(ARM_UNSTOWED_POS); mask += ARM_CMD_INDS
            if self.use_gripper:
                vals.append(0.0)
                self.gripper_selection_index = len(vals) - 1
        if self.use_legs:
            vals += [*LEGS_STANDING_POS[0:6], 0]; mask += FRONT_LEG_CMD_INDS
            self.leg_selection_index = len(vals) - 1
        if self.use_torso:
            vals += [0, 0, STANDING_HEIGHT]; mask += TORSO_CMD_INDS
        self.default_command = np.array(vals, dtype=np.float64)
        self.command_mask = np.array(mask)

    # ---- command mapping ---------------------------------------------------------------------------------------------------
    def apply_selection_mask(self, controls):
        """:265-331.  Leg selection in [-1, -0.5) keeps the front-left leg command, (0.5, 1] the front-right, otherwise neither;
        gripper selection < 0 closes the gripper.  The selection entries are removed from the result."""
        if self.leg_selection_index is None and self.gripper_selection_index is None:
            return controls
        tor = _is_torch(controls)
        added = controls.ndim == 1
        c = (controls.clone() if tor else np.array(controls, copy=True))
        if added:
            c = c[None]
        if self.use_arm and self.use_gripper and self.gripper_selection_index is not None:
            closed = c[..., self.gripper_selection_index] < 0.0
            c[..., 9] = (c[..., 9].masked_fill(closed, GRIPPER_CLOSED_POS) if tor else np.where(closed, GRIPPER_CLOSED_POS, c[..., 9]))
        if self.use_legs and self.leg_selection_index is not None:
            sel = c[..., self.leg_selection_index]
            keep_fl, keep_fr = sel < -0.5, sel > 0.5
            s0 = 3 + ((7 + (1 if self.use_gripper else 0)) if self.use_arm else 0)
            kf = keep_fl[..., None].to(c.dtype) if tor else keep_fl[..., None].astype(c.dtype)
            kr = keep_fr[..., None].to(c.dtype) if tor else keep_fr[..., None].astype(c.dtype)
            c[..., s0 : s0 + 3] = c[..., s0 : s0 + 3] * kf
            c[..., s0 + 3 : s0 + 6] = c[..., s0 + 3 : s0 + 6] * kr
        keep = [i for i in range(c.shape[-1]) if i not in (self.leg_selection_index, self.gripper_selection_index)]
        c = c[..., keep]
        return c[0] if added else c

    def task_to_sim_ctrl(self, controls):
        """:325-391: (..., nu) compact controls -> (..., 25) policy commands [base vel 3 | arm 7 | leg override 12 | torso roll, pitch, height].
        Shapes as the reference returns them: (N, T, nu) -> (N, T, 25); (N, nu) -> (N, 25); (nu,) -> (1, 25); and (N, 1, nu) -> (N, 25) (its
        single-timestep squeeze, :386-387)."""
        tor = _is_torch(controls)
        c = controls if tor else np.asarray(controls)
        shape_in = c.shape
        c = self.apply_selection_mask(c[None] if c.ndim == 1 else c)
        if tor:
            import torch

            out = torch.as_tensor(self.default_policy_command, dtype=c.dtype, device=c.device).expand(*c.shape[:-1], 25).clone()
        else:
            out = np.broadcast_to(self.default_policy_command, (*c.shape[:-1], 25)).copy()
        arm_end = 3 + (7 if self.use_arm else 0)
        legs_end = arm_end + (6 if self.use_legs else 0)
        out[..., 0:3] = c[..., 0:3]
        if self.use_arm:
            out[..., 3:10] = c[..., 3:arm_end]
        if self.use_legs:
            out[..., 10:16] = c[..., arm_end:legs_end]
        if self.use_torso:
            out[..., 22:25] = c[..., legs_end : legs_end + 3]
        if len(shape_in) == 3 and shape_in[1] == 1:
            return out[:, 0, :]
        return out

    # ---- reward / reset ------------------------------------------------------------------------------------------------------
    def reward(self, states, sensors, controls, system_metadata: dict[str, Any] | None = None):   # :393-414
        if _is_torch(states):
            import torch

            return torch.zeros(states.shape[0], dtype=states.dtype, device=states.device)
        return np.zeros(states.shape[0])

    @property
    def reset_arm_pos(self) -> np.ndarray:   # :416-419
        return ARM_UNSTOWED_POS if self.use_arm else ARM_STOWED_POS

    @property
    def reset_pose(self) -> np.ndarray:      # :421-435
        return np.array([0.0, 0.0, STANDING_HEIGHT, 1, 0, 0, 0, *LEGS_STANDING_POS_RL, *self.reset_arm_pos])

    def reset(self) -> None:                 # :437-441
        self.data.qpos = np.array(self.reset_pose, dtype=np.float64)
        self.data.qvel = np.zeros(self.nv)

    def get_action_components(self) -> list[str]:   # :443-461
        names = ["spot/base.vx", "spot/base.vy", "spot/base.vtheta"]
        if self.use_arm:
            names += [f"spot/{j}" for j in ("arm_sh0", "arm_sh1", "arm_el0", "arm_el1", "arm_wr0", "arm_wr1", "arm_f1x")]
        if self.use_legs:
            names += [f"spot/{j}" for j in ("fr_hx", "fr_hy", "fr_kn", "fl_hx", "fl_hy", "fl_kn")] + ["spot/leg_selection"]
        if self.use_torso:
            names += ["spot/torso.roll", "spot/torso.pitch", "spot/torso.height"]
        return names


@dataclass
class SpotNavigateConfig(SpotBaseConfig):   # spot_navigate.py:19-33
    w_goal: float = 60.0
    fall_penalty: float = 2500.0
    w_controls: float = 0.0
    goal_position: np.ndarray = field(default_factory=lambda: np.array([0.0, 0.0, STANDING_HEIGHT]))


class SpotNavigate(SpotBase):
    """spot_navigate.py:36-82: walk the base to a goal position; base-velocity commands only."""

    name = "spot_navigate"
    config_t = SpotNavigateConfig

    def __init__(self, config: SpotNavigateConfig | None = None) -> None:
        super().__init__(use_arm=False, config=config)
        self.body_pose_idx = 0

    def reward(self, states, sensors, controls, system_metadata: dict[str, Any] | None = None):   # :50-77
        cfg = self.config
        i = self.body_pose_idx
        if _is_torch(states):
            import torch

            pos = states[..., i : i + 3]
            goal = torch.as_tensor(np.asarray(cfg.goal_position), dtype=states.dtype, device=states.device)
            fallen = (states[..., i + 2] <= cfg.spot_fallen_threshold).any(dim=-1).to(states.dtype)
            r = -cfg.fall_penalty * fallen - cfg.w_goal * torch.linalg.norm(pos - goal, dim=-1).mean(-1)
            return r - cfg.w_controls * torch.linalg.norm(controls, dim=-1).mean(-1)
        pos = states[..., i : i + 3]
        fallen = (states[..., i + 2] <= cfg.spot_fallen_threshold).any(axis=-1)
        r = -cfg.fall_penalty * fallen - cfg.w_goal * np.linalg.norm(pos - np.asarray(cfg.goal_position)[None, None], axis=-1).mean(-1)
        return r - cfg.w_controls * np.linalg.norm(controls, axis=-1).mean(-1)

    @property
    def reset_pose(self) -> np.ndarray:     # :79-82
        return np.array([0, 0, STANDING_HEIGHT, 1, 0, 0, 0, *LEGS_STANDING_POS, *self.reset_arm_pos])


# ---- judo/tasks/spot/spot_box_push.py ---------------------------------------------------------------------------------
RADIUS_MIN, RADIUS_MAX = 1.0, 2.0           # :21-22


@dataclass
class SpotBoxPushConfig(SpotBaseConfig):    # spot_box_push.py:25-45
    w_goal: float = 60.0
    w_orientation: float = 15.0
    w_torso_proximity: float = 0.1
    w_gripper_proximity: float = 4.0
    orientation_threshold: float = 0.5
    fall_penalty: float = 2500.0
    w_controls: float = 0.0
    goal_position: np.ndarray = field(default_factory=lambda: np.array([0.0, 0.0, BOX_HALF_LENGTH]))


class SpotBoxPush(SpotBase):
    """spot_box_push.py:48-127: push the box to a goal position with the arm unstowed.  The model is `spot_box` (judo_amd.models.spot_box_description)."""

    name = "spot_box_push"
    model_name = "spot_box"
    config_t = SpotBoxPushConfig

    def __init__(self, config: SpotBoxPushConfig | None = None) -> None:
        super().__init__(use_arm=True, config=config)
        self.body_pose_idx = self.get_joint_position_start_index("base")
        self.object_pose_idx = self.get_joint_position_start_index("box_joint")
        self.object_y_axis_idx = self.get_sensor_start_index("object_y_axis")
        self.gripper_pos_idx = self.get_sensor_start_index("trace_fngr_site")

    def reward(self, states, sensors, controls, system_metadata: dict[str, Any] | None = None):   # :70-115
        """As the reference computes it: the torso term enters with a POSITIVE sign, the orientation term counts the steps whose object y axis points up
        (y . z > threshold), every other term is a mean over time."""
        cfg = self.config
        b, o, y, gi = self.body_pose_idx, self.object_pose_idx, self.object_y_axis_idx, self.gripper_pos_idx
        body_height, body_pos, object_pos = states[..., b + 2], states[..., b : b + 3], states[..., o : o + 3]
        object_y_axis, gripper_pos = sensors[..., y : y + 3], sensors[..., gi : gi + 3]
        if _is_torch(states):
            import torch

            goal = torch.as_tensor(np.asarray(cfg.goal_position), dtype=states.dtype, device=states.device)
            fallen = -cfg.fall_penalty * (body_height <= cfg.spot_fallen_threshold).any(dim=-1).to(states.dtype)
            r = fallen - cfg.w_goal * torch.linalg.norm(object_pos - goal, dim=-1).mean(-1)
            r = r - cfg.w_orientation * (object_y_axis[..., 2] > cfg.orientation_threshold).to(states.dtype).sum(-1)
            r = r + cfg.w_torso_proximity * torch.linalg.norm(body_pos - object_pos, dim=-1).mean(-1)
            r = r - cfg.w_gripper_proximity * torch.linalg.norm(gripper_pos - object_pos, dim=-1).mean(-1)
            return r - cfg.w_controls * torch.linalg.norm(controls, dim=-1).mean(-1)
        fallen = -cfg.fall_penalty * (body_height <= cfg.spot_fallen_threshold).any(axis=-1)
        r = fallen - cfg.w_goal * np.linalg.norm(object_pos - np.asarray(cfg.goal_position)[None, None], axis=-1).mean(-1)
        r = r - cfg.w_orientation * np.abs(np.dot(object_y_axis, Z_AXIS) > cfg.orientation_threshold).sum(axis=-1)
        r = r + cfg.w_torso_proximity * np.linalg.norm(body_pos - object_pos, axis=-1).mean(-1)
        r = r - cfg.w_gripper_proximity * np.linalg.norm(gripper_pos - object_pos, axis=-1).mean(-1)
        return r - cfg.w_controls * np.linalg.norm(controls, axis=-1).mean(-1)

    def default_state(self) -> np.ndarray:
        """Deterministic x0 for the benchmark / parity harness: the robot standing at the origin with the arm unstowed, the box 1.5 m ahead, at rest."""
        return np.concatenate([[0, 0, STANDING_HEIGHT, 1, 0, 0, 0], LEGS_STANDING_POS, self.reset_arm_pos, [1.5, 0, BOX_HALF_LENGTH, 1, 0, 0, 0], np.zeros(self.nv)])

    @property
    def reset_pose(self) -> np.ndarray:     # :117-127: base at randn(2), the box at radius 1..2 in a random direction plus randn(2)
        radius = RADIUS_MIN + (RADIUS_MAX - RADIUS_MIN) * np.random.rand()
        theta = 2 * np.pi * np.random.rand()
        object_xy = np.array([radius * np.cos(theta), radius * np.sin(theta)]) + np.random.randn(2)
        reset_object_pose = np.array([*object_xy, BOX_HALF_LENGTH, 1, 0, 0, 0])
        return np.array([*np.random.randn(2), STANDING_HEIGHT, 1, 0, 0, 0, *LEGS_STANDING_POS, *self.reset_arm_pos, *reset_object_pose])


# ---- judo/tasks/spot/spot_tire_roll.py, spot_tire_upright.py ------------------------------------------------------------
def _apply_quat_to_vec(quat, vec):  # judo/tasks/spot/spot_utils.py:8-23
    w, xyz = quat[..., 0:1], quat[..., 1:4]
    if _is_torch(vec):
        import torch

        t = 2.0 * torch.linalg.cross(xyz.expand_as(vec), vec, dim=-1)
        return vec + w * t + torch.linalg.cross(xyz.expand_as(t), t, dim=-1)
    t = 2.0 * np.cross(xyz, vec)
    return vec + w * t + np.cross(xyz, t)


def _tire_state(task, x_tire) -> np.ndarray:
    """The robot standing at the origin with the task's reset arm, the tire at `x_tire` (position, quaternion), everything at rest."""
    return np.concatenate([[0, 0, STANDING_HEIGHT, 1, 0, 0, 0], LEGS_STANDING_POS, task.reset_arm_pos, x_tire, np.zeros(task.nv)])


@dataclass
class SpotTireRollConfig(SpotBaseConfig):   # spot_tire_roll.py:27-49
    fall_penalty: float = 5000.0
    tire_fallen_threshold: float = 0.1
    w_goal: float = 60.0
    w_torso_proximity: float = 1.0
    torso_goal_offset: float = 1.0
    w_gripper_proximity: float = 1.0
    gripper_goal_offset: float = 0.15
    gripper_goal_altitude: float = 0.05
    w_tire_linear_velocity: float = 10.0
    w_tire_angular_velocity: float = 0.30
    w_controls: float = 0.0
    goal_position: np.ndarray = field(default_factory=lambda: np.array([0.0, 0.0, TIRE_RADIUS]))


class SpotTireRoll(SpotBase):
    """spot_tire_roll.py:52-151: roll the tire to a goal position, arm and gripper in the command.  The model is `spot_tire` (judo_amd.models.spot_tire_description)."""

    name = "spot_tire_roll"
    model_name = "spot_tire"
    config_t = SpotTireRollConfig

    def __init__(self, config: SpotTireRollConfig | None = None) -> None:
        super().__init__(use_arm=True, use_gripper=True, config=config)
        self.body_pose_idx = self.get_joint_position_start_index("base")
        self.object_pose_idx = self.get_joint_position_start_index("tire_joint")
        self.gripper_pos_idx = self.get_sensor_start_index("trace_fngr_site")
        self.object_y_axis_idx = self.get_sensor_start_index("object_y_axis")
        self.object_vel_idx = 25                 # jnt_dofadr of tire_joint: after the robot's 25 dofs

    def reward(self, states, sensors, controls, system_metadata: dict[str, Any] | None = None):   # :73-137
        """As the reference computes it: the tire-fallen term COUNTS the steps whose y axis leans out of the horizontal (|y . z| > threshold) and multiplies the count by
        the fall penalty; the gripper goal sits at a fixed altitude; every other term is a mean over time."""
        cfg, nq = self.config, self.nq
        b, o, gi, y, v = self.body_pose_idx, self.object_pose_idx, self.gripper_pos_idx, self.object_y_axis_idx, nq + self.object_vel_idx
        body_height, body_pos, object_pos = states[..., b + 2], states[..., b : b + 3], states[..., o : o + 3]
        tire_lin, tire_ang = states[..., v : v + 3], states[..., v + 3 : v + 6]
        gripper_pos, object_y_axis = sensors[..., gi : gi + 3], sensors[..., y : y + 3]
        if _is_torch(states):
            import torch

            goal = torch.as_tensor(np.asarray(cfg.goal_position), dtype=states.dtype, device=states.device)
            to_goal = goal - object_pos
            direction = to_goal / (1e-2 + torch.linalg.norm(to_goal, dim=-1, keepdim=True))
            gripper_goal = object_pos - cfg.gripper_goal_offset * direction
            gripper_goal = torch.cat([gripper_goal[..., :2], torch.full_like(gripper_goal[..., 2:], cfg.gripper_goal_altitude)], dim=-1)
            torso_goal = object_pos - cfg.torso_goal_offset * direction
            r = -cfg.fall_penalty * (body_height <= cfg.spot_fallen_threshold).any(dim=-1).to(states.dtype)
            r = r - cfg.fall_penalty * (object_y_axis[..., 2] > cfg.tire_fallen_threshold).to(states.dtype).sum(-1)
            r = r - cfg.w_goal * torch.linalg.norm(object_pos - goal, dim=-1).mean(-1)
            r = r - cfg.w_torso_proximity * torch.linalg.norm(body_pos - torso_goal, dim=-1).mean(-1)
            r = r - cfg.w_gripper_proximity * torch.linalg.norm(gripper_goal - gripper_pos, dim=-1).mean(-1)
            r = r - cfg.w_controls * torch.linalg.norm(controls, dim=-1).mean(-1)
            r = r - cfg.w_tire_linear_velocity * torch.linalg.norm(tire_lin, dim=-1).mean(-1)
            return r - cfg.w_tire_angular_velocity * torch.linalg.norm(tire_ang, dim=-1).mean(-1)
        goal = np.asarray(cfg.goal_position)
        to_goal = goal - object_pos
        direction = to_goal / (1e-2 + np.linalg.norm(to_goal, axis=-1, keepdims=True))
        gripper_goal = object_pos - cfg.gripper_goal_offset * direction
        gripper_goal[..., 2] = cfg.gripper_goal_altitude
        torso_goal = object_pos - cfg.torso_goal_offset * direction
        r = -cfg.fall_penalty * (body_height <= cfg.spot_fallen_threshold).any(axis=-1)
        r = r - cfg.fall_penalty * np.abs(np.dot(object_y_axis, Z_AXIS) > cfg.tire_fallen_threshold).sum(axis=-1)
        r = r - cfg.w_goal * np.linalg.norm(object_pos - goal, axis=-1).mean(-1)
        r = r - cfg.w_torso_proximity * np.linalg.norm(body_pos - torso_goal, axis=-1).mean(-1)
        r = r - cfg.w_gripper_proximity * np.linalg.norm(gripper_goal - gripper_pos, axis=-1).mean(-1)
        r = r - cfg.w_controls * np.linalg.norm(controls, axis=-1).mean(-1)
        r = r - cfg.w_tire_linear_velocity * np.linalg.norm(tire_lin, axis=-1).mean(-1)
        return r - cfg.w_tire_angular_velocity * np.linalg.norm(tire_ang, axis=-1).mean(-1)

    def default_state(self) -> np.ndarray:
        """Deterministic x0 for the benchmark / parity harness: the robot standing at the origin, the tire upright 1.5 m ahead (its axis across the line to it), at rest."""
        return _tire_state(self, [1.5, 0, TIRE_RADIUS, 1, 0, 0, 0])

    @property
    def reset_pose(self) -> np.ndarray:     # :139-151: the tire upright at a uniform position in [-1.5, 1.5]^2, at least 1 m from the robot's standing point
        standing_pose = np.array([0, 0, STANDING_HEIGHT])
        reset_pose = (np.random.rand(7) - 0.5) * 3.0
        reset_pose[2] = TIRE_RADIUS
        reset_pose[3:] = [1, 0, 0, 0]
        while np.linalg.norm(reset_pose[:3] - standing_pose) < 1.0:
            reset_pose = (np.random.rand(7) - 0.5) * 3.0
            reset_pose[2] = TIRE_RADIUS
            reset_pose[3:] = [1, 0, 0, 0]
        return np.array([*standing_pose, 1, 0, 0, 0, *LEGS_STANDING_POS, *self.reset_arm_pos, *reset_pose])


@dataclass
class SpotTireUprightConfig(SpotBaseConfig):   # spot_tire_upright.py:24-44
    orientation_error_smoothing_width: float = 1.0
    w_tire_orientation: float = 200.0
    w_gripper_proximity: float = 10.0
    w_foot_proximity: float = 5.0
    w_torso_proximity: float = 5.0
    gripper_too_inside_tire_penalty: float = 150.0
    gripper_not_above_tire_penalty: float = 100.0
    w_controls: float = 2.0
    fall_penalty: float = 10_000.0


class SpotTireUpright(SpotBase):
    """spot_tire_upright.py:47-334: stand a flat tire up with the arm and the front legs (use_legs=True, use_gripper=False: the legs' six commands follow the arm's
    seven).  The model is `spot_tire`."""

    name = "spot_tire_upright"
    model_name = "spot_tire"
    config_t = SpotTireUprightConfig
    _YAW = np.array([np.cos(np.pi / 8), 0, 0, np.sin(np.pi / 8)])           # :145, the right foot's goal direction
    _YAW_NEG = np.array([np.cos(np.pi / 8), 0, 0, np.sin(-np.pi / 8)])      # :151, the left foot's

    def __init__(self, config: SpotTireUprightConfig | None = None) -> None:
        super().__init__(use_arm=True, use_gripper=False, use_legs=True, use_torso=False, config=config)
        self.body_pose_idx = self.get_joint_position_start_index("base")
        self.object_pose_idx = self.get_joint_position_start_index("tire_joint")
        self.tire_y_axis_idx = self.get_sensor_start_index("object_y_axis")
        self.gripper_pos_idx = self.get_sensor_start_index("trace_fngr_site")
        self.fl_pos_idx = self.get_sensor_start_index("fl_pos")
        self.fr_pos_idx = self.get_sensor_start_index("fr_pos")

    def reward(self, states, sensors, controls, system_metadata: dict[str, Any] | None = None):   # :99-235
        """As the reference computes it: the BETTER (max) of the two foot terms, the orientation term exp(|y_z| / width) (1 .. e), the gripper penalties as fractions
        of the horizon, the fall penalty once per rollout."""
        cfg = self.config
        o, b, y, gi, fl, fr = self.object_pose_idx, self.body_pose_idx, self.tire_y_axis_idx, self.gripper_pos_idx, self.fl_pos_idx, self.fr_pos_idx
        p_tire, p_torso = states[..., o : o + 3], states[..., b : b + 3]
        p_grip, p_fr, p_fl, tire_y = sensors[..., gi : gi + 3], sensors[..., fr : fr + 3], sensors[..., fl : fl + 3], sensors[..., y : y + 3]
        tt = _is_torch(states)
        if tt:
            import torch

            norm = lambda v: torch.linalg.norm(v, dim=-1)   # noqa: E731
            quat = lambda q: torch.as_tensor(q, dtype=states.dtype, device=states.device)   # noqa: E731
            setz = lambda v, z: torch.cat([v[..., :2], torch.full_like(v[..., 2:], z)], dim=-1)   # noqa: E731
            fdt = lambda m: m.to(states.dtype)   # noqa: E731
        else:
            norm = lambda v: np.linalg.norm(v, axis=-1)   # noqa: E731
            quat = lambda q: q   # noqa: E731

            def setz(v, z):
                v = v.copy()
                v[..., 2] = z
                return v

            fdt = lambda m: m   # noqa: E731
        d = p_torso - p_tire
        u = d / (norm(d)[..., None] + 1e-8)
        grip_des = setz(p_tire + (TIRE_RADIUS - 0.05) * u, TIRE_HALF_WIDTH + 0.1)
        gripper_proximity = -cfg.w_gripper_proximity * norm(p_grip - grip_des).mean(-1)
        right_des = setz(p_tire + TIRE_RADIUS * _apply_quat_to_vec(quat(self._YAW), u), 0.1)
        left_des = setz(p_tire + TIRE_RADIUS * _apply_quat_to_vec(quat(self._YAW_NEG), u), 0.1)
        right = -cfg.w_foot_proximity * norm(p_fr - right_des).mean(-1)
        left = -cfg.w_foot_proximity * norm(p_fl - left_des).mean(-1)
        foot_proximity = torch.maximum(right, left) if tt else np.maximum(right, left)
        torso_proximity = -cfg.w_torso_proximity * norm(p_torso - setz(p_tire + 0.75 * u, STANDING_HEIGHT)).mean(-1)
        err = tire_y[..., 2].abs() if tt else np.abs(tire_y[..., 2])
        orientation = -cfg.w_tire_orientation * ((err / cfg.orientation_error_smoothing_width).exp() if tt else np.exp(err / cfg.orientation_error_smoothing_width)).mean(-1)
        dist = norm(p_grip - p_tire)
        inside = -cfg.gripper_too_inside_tire_penalty * fdt(dist < TIRE_RADIUS * 0.5).mean(-1)
        not_above = (p_grip[..., 2] < 2 * TIRE_HALF_WIDTH + 0.05) & (dist > TIRE_RADIUS)
        not_above_r = -cfg.gripper_not_above_tire_penalty * fdt(not_above).mean(-1)
        fallen = states[..., b + 2] <= cfg.spot_fallen_threshold
        fallen_r = -cfg.fall_penalty * (fdt(fallen.any(dim=-1)) if tt else fallen.any(axis=-1))
        controls_r = -cfg.w_controls * norm(controls).mean(-1)
        return orientation + gripper_proximity + foot_proximity + torso_proximity + inside + not_above_r + fallen_r + controls_r

    def success(self, sensordata, metadata: dict[str, Any] | None = None) -> bool:   # :315-334: the tire's y axis horizontal within 0.1
        return bool(abs(float(np.asarray(sensordata)[self.tire_y_axis_idx + 2])) <= 0.1)

    def default_state(self) -> np.ndarray:
        """Deterministic x0 for the benchmark / parity harness: the robot standing at the origin, the tire lying flat 1.5 m ahead (the reset's fallback pose), at rest."""
        return _tire_state(self, [1.5, 0, TIRE_HALF_WIDTH, np.cos(np.pi / 4), np.sin(np.pi / 4), 0, 0])

    @property
    def reset_pose(self) -> np.ndarray:     # :237-312: the tire flat (rolled +-90 degrees, random yaw) in [-2, 2]^2, the robot at a random pose more than 1 m away
        for _ in range(100):
            tire_x, tire_y = np.random.uniform(-2, 2), np.random.uniform(-2, 2)
            tire_quat = np.array([1 / np.sqrt(2), 1 / np.sqrt(2), 0, 0]) if np.random.random() < 0.5 else np.array([1 / np.sqrt(2), -1 / np.sqrt(2), 0, 0])
            yaw = np.random.uniform(0, 2 * np.pi)
            w1, x1, y1, z1 = np.cos(yaw / 2), 0, 0, np.sin(yaw / 2)
            w2, x2, y2, z2 = tire_quat
            q = np.array([w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2, w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2, w1 * y2 - x1 * z2 + y1 * w2 + z1 * x2, w1 * z2 + x1 * y2 - y1 * x2 + z1 * w2])
            robot_x, robot_y = np.random.uniform(-2, 2), np.random.uniform(-2, 2)
            yaw_r = np.random.uniform(0, 2 * np.pi)
            robot_quat = np.array([np.cos(yaw_r / 2), 0, 0, np.sin(yaw_r / 2)])
            if np.linalg.norm(np.array([robot_x, robot_y]) - np.array([tire_x, tire_y])) > 1.0:
                return np.array([robot_x, robot_y, STANDING_HEIGHT, *robot_quat, *LEGS_STANDING_POS, *self.reset_arm_pos, tire_x, tire_y, TIRE_HALF_WIDTH, *q])
        return np.array([0.0, 0.0, STANDING_HEIGHT, 1, 0, 0, 0, *LEGS_STANDING_POS, *self.reset_arm_pos, 2.0, 0.0, TIRE_HALF_WIDTH, np.cos(np.pi / 4), np.sin(np.pi / 4), 0, 0])


register_task(SpotBase.name, SpotBase, SpotBaseConfig)
register_task(SpotNavigate.name, SpotNavigate, SpotNavigateConfig)
register_task(SpotBoxPush.name, SpotBoxPush, SpotBoxPushConfig)
register_task(SpotTireRoll.name, SpotTireRoll, SpotTireRollConfig)
register_task(SpotTireUpright.name, SpotTireUpright, SpotTireUprightConfig)
