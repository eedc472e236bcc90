"""Model constants for the rollout kernels (host side).

`load_description(task)` reads `judo_amd/models/<task>.json` -- the numbers of the reference's MJCF
(judo/models/xml/{cartpole,cylinder_push,leap_cube,fr3_pick}.xml) transcribed
into this build's schema by tools/compile_mjcf.py.  `pack_model(desc)` derives the constants the kernels need
(what MuJoCo's compiler would precompute: inverse weights at the reference pose `qpos0`, solref -> (K, B) with
the refsafe clamp, candidate collision pairs) and serialises them into the blob `jh_model_create` uploads.

This is the product's own host code: numpy only, no oracle, no MuJoCo.
"""

from __future__ import annotations

import copy
import json
import os
import struct
from dataclasses import dataclass

import numpy as np

MODEL_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "models")
TASK_KIND = {"cartpole": 0, "cylinder_push": 1, "leap_cube": 2, "fr3_pick": 3}
BLOB_MAGIC = 0x314D484A
MINVAL = 1e-15
MINMU = 1e-5


def load_description(task: str) -> dict:
    if task in DERIVED_DESCRIPTIONS:
        return DERIVED_DESCRIPTIONS[task]()
    path = os.path.join(MODEL_DIR, task + ".json")
    if not os.path.exists(path):
        raise ValueError(f"unknown task {task!r}: no model description at {path}")
    with open(path) as f:
        return json.load(f)


def spot_box_description() -> dict:
    """The Spot robot with a free box (judo/models/xml/spot_box/robot.xml), derived from `spot.json` rather than transcribed into a file of its own.

    spot_box/robot.xml includes the same spot_primitive/{default,body,legs,arm,actuator,contact}.xml as spot_primitive/robot.xml, so the robot's
    bodies, joints, geoms, actuators and excludes are spot.json's.  What differs:
      * the robot's body sits at z = 0.52 (robot.xml:16; spot_primitive: 0.7).  This moves qpos0 only: the inverse weights at qpos0 of the free base
        (and of every body) do not depend on where the whole robot stands, the mass matrix being expressed about the base;
      * a body `box_body` (robot.xml:22) with a free joint `box_joint` (:23), inertia at its origin (:24: mass 1.5, diaginertia 0.1445 x 3), a box geom
        `box_collision` (:25: half size 0.254, class "collision" -> friction 0.15 and MuJoCo's default solref / solimp, the values every robot geom carries,
        spot_primitive/default.xml:14-17; priority 4), and the site `site_object` (:27) that spot_primitive declares in the world body;
      * the sensor list of robot.xml:36-50 (13 world-frame site sensors, 39 floats; no reference frames).
    Bodies and geoms are in the order the MJCF compiler gives them (tools/compile_mjcf.py transcribes the XML to the same description): the box body
    before the static fixtures that hold the plane, the box geom before the plane."""
    d = load_description("spot")
    bodies, geoms, sites = d["bodies"], d["geoms"], d["sites"]
    fix = next(i for i, b in enumerate(bodies) if b["name"] == "world_fixtures")
    assert fix == len(bodies) - 1 and all(b["parent"] != fix for b in bodies)
    box = fix                                                   # the box takes the fixtures' index, the fixtures move one up
    for g in geoms:
        g["body"] = g["body"] + 1 if g["body"] == fix else g["body"]
    for st in sites:
        st["body"] = st["body"] + 1 if st["body"] == fix else st["body"]
    bodies[1] = dict(bodies[1], pos=[0.0, 0.0, 0.52])                                                         # robot.xml:16
    bodies.insert(box, dict(name="box_body", parent=0, pos=[2.0, 0.0, 0.254], quat=[1.0, 0.0, 0.0, 0.0], mocap=False,   # :22
                            mass=1.5, ipos=[0.0, 0.0, 0.0], iquat=[1.0, 0.0, 0.0, 0.0], inertia=[0.1445, 0.1445, 0.1445]))   # :24
    base = next(j for j in d["joints"] if j["type"] == "free")
    d["joints"].append(dict(base, name="box_joint", body=box))                                               # :23 (a free joint's defaults, as the base's)
    robot = next(g for g in geoms if g["type"] != "plane")      # class "collision": the contact parameters every robot geom carries
    plane = next(i for i, g in enumerate(geoms) if g["type"] == "plane")
    geoms.insert(plane, dict(name="box_collision", body=box, type="box", condim=robot["condim"], friction=list(robot["friction"]), solref=list(robot["solref"]),   # :25
                             solimp=list(robot["solimp"]), margin=robot["margin"], gap=robot["gap"], solmix=robot["solmix"], priority=4, pos=[0.0, 0.0, 0.0],
                             quat=[1.0, 0.0, 0.0, 0.0], size=[0.254, 0.254, 0.254]))
    obj = next(i for i, st in enumerate(sites) if st["name"] == "site_object")
    sites[obj] = dict(sites[obj], body=box, pos=[0.0, 0.0, 0.0])                                              # :27
    site = {st["name"]: i for i, st in enumerate(sites)}
    sens = [("sensor_body", "framepos", "site_body"), ("body_x_axis", "framexaxis", "site_body"), ("object_x_axis", "framexaxis", "site_object"),   # :37-39
            ("object_y_axis", "frameyaxis", "site_object"), ("object_z_axis", "framezaxis", "site_object"), ("trace_fngr_site", "framepos", "site_arm_link_fngr"),   # :40-42
            ("gripper_x_axis", "framexaxis", "site_arm_link_wr1"), ("gripper_y_axis", "frameyaxis", "site_arm_link_wr1"), ("finger_x_axis", "framexaxis", "site_arm_link_fngr"),   # :43-45
            ("fl_pos", "framepos", "site_front_left"), ("fr_pos", "framepos", "site_front_right"), ("hl_pos", "framepos", "site_rear_left"), ("hr_pos", "framepos", "site_rear_right")]   # :46-49
    d["sensors"] = [dict(name=n, type=t, adr=3 * k, objtype="site", obj=site[s], dim=3) for k, (n, t, s) in enumerate(sens)]
    d["nsensordata"] = 3 * len(sens)
    d["task"], d["family"], d["source"] = "spot_box", "spot", "judo v0.0.7 judo/models/xml/spot_box/robot.xml (derived from spot.json)"
    return d


def spot_tire_description() -> dict:
    """The Spot robot with a free tire (judo/models/xml/spot_tire/robot.xml + objects/tire/tire.xml), derived from `spot.json` as `spot_box` is.

    spot_tire/robot.xml restates spot_primitive's default classes and includes its body / legs / arm / actuator / contact files, so the robot is spot.json's,
    standing at z = 0.52 (robot.xml:79).  What the tire adds (tire.xml):
      * a body `tire` (:4, at the origin) with a free joint `tire_joint` (:5), inertia at its origin (:7: mass 15.3, diaginertia 0.57 0.96 0.57), and the sites
        `trace_tire` and `site_object` (:93-95) at its origin;
      * ONE collision geom, a STAND-IN: the reference collides the tire through 81 convex meshes that it does not ship.  The stand-in is the
        reference's own primitive approximation `object_primitive_approx` (:9: a cylinder of radius 0.33 and half-length 0.17, quat 1 1 0 0 = its axis along the
        body's y axis; TIRE_RADIUS / TIRE_HALF_WIDTH, spot_constants.py:123-124), made collidable with the meshes' class `tire_collision` (tire_defs.xml:9:
        friction 1.15 1.0, priority 6 -- above the robot's 4 and the ground's 5, so the tire's friction and solver parameters win in every pair).
      * the sensor list of robot.xml:95-116: 20 site sensors, 60 floats, all in the WORLD frame (spot.json's sensor_arm_link_* are relative to site_body).
    Bodies and geoms in the MJCF compiler's order: the tire body before the fixtures that hold the plane, its geom before the plane."""
    d = load_description("spot")
    bodies, geoms, sites = d["bodies"], d["geoms"], d["sites"]
    fix = next(i for i, b in enumerate(bodies) if b["name"] == "world_fixtures")
    assert fix == len(bodies) - 1 and all(b["parent"] != fix for b in bodies)
    tire = fix
    for g in geoms:
        g["body"] = g["body"] + 1 if g["body"] == fix else g["body"]
    bodies[1] = dict(bodies[1], pos=[0.0, 0.0, 0.52])
    bodies.insert(tire, dict(name="tire", parent=0, pos=[0.0, 0.0, 0.0], quat=[1.0, 0.0, 0.0, 0.0], mocap=False,
                             mass=15.3, ipos=[0.0, 0.0, 0.0], iquat=[1.0, 0.0, 0.0, 0.0], inertia=[0.57, 0.96, 0.57]))
    base = next(j for j in d["joints"] if j["type"] == "free")
    d["joints"].append(dict(base, name="tire_joint", body=tire))
    robot = next(g for g in geoms if g["type"] != "plane")
    plane = next(i for i, g in enumerate(geoms) if g["type"] == "plane")
    h = 1.0 / float(np.sqrt(2.0))                                # (quat 1 1 0 0, normalised as the MJCF compiler does)
    geoms.insert(plane, dict(name="object_primitive_approx", body=tire, type="cylinder", condim=robot["condim"], friction=[1.15, 1.0, 0.0001],
                             solref=list(robot["solref"]), solimp=list(robot["solimp"]), margin=0.0, gap=0.0, solmix=1.0, priority=6, pos=[0.0, 0.0, 0.0],
                             quat=[h, h, 0.0, 0.0], size=[0.33, 0.17]))
    obj = next(i for i, st in enumerate(sites) if st["name"] == "site_object")
    site_object = dict(sites.pop(obj), body=tire, pos=[0.0, 0.0, 0.0])
    sites += [dict(site_object, name="trace_tire"), site_object]
    site = {st["name"]: i for i, st in enumerate(sites)}
    sens = [("sensor_body", "framepos", "site_body"), ("body_x_axis", "framexaxis", "site_body"), ("object_x_axis", "framexaxis", "site_object"),
            ("object_y_axis", "frameyaxis", "site_object"), ("object_z_axis", "framezaxis", "site_object"), ("trace_fngr_site", "framepos", "site_arm_link_fngr"),
            ("gripper_x_axis", "framexaxis", "site_arm_link_wr1"), ("gripper_y_axis", "frameyaxis", "site_arm_link_wr1"), ("finger_x_axis", "framexaxis", "site_arm_link_fngr"),
            ("fl_pos", "framepos", "site_front_left"), ("fr_pos", "framepos", "site_front_right"), ("hl_pos", "framepos", "site_rear_left"), ("hr_pos", "framepos", "site_rear_right")]
    sens += [(f"sensor_arm_link_{n}", "framepos", f"site_arm_link_{n}") for n in ("sh0", "sh1", "el0", "el1", "wr0", "wr1", "fngr")]
    d["sensors"] = [dict(name=n, type=t, adr=3 * k, objtype="site", obj=site[s], dim=3) for k, (n, t, s) in enumerate(sens)]
    d["nsensordata"] = 3 * len(sens)
    d["task"], d["family"], d["source"] = "spot_tire", "spot", "judo v0.0.7 judo/models/xml/spot_tire/robot.xml (derived from spot.json; cylinder stand-in for the tire's meshes)"
    return d


DERIVED_DESCRIPTIONS = {"spot_box": spot_box_description, "spot_tire": spot_tire_description}


# ----------------------------------------------------------------------------------------- small rigid-body helpers
def quat_to_mat(q) -> np.ndarray:
    w, x, y, z = q
    return np.array(
        [
            [1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
            [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
            [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)],
        ]
    )


def quat_mul(a, b) -> np.ndarray:
    return np.array(
        [
            a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3],
            a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2],
            a[0] * b[2] - a[1] * b[3] + a[2] * b[0] + a[3] * b[1],
            a[0] * b[3] + a[1] * b[2] - a[2] * b[1] + a[3] * b[0],
        ]
    )


@dataclass
class Layout:
    """Index bookkeeping of a description (MuJoCo ordering: joints/dofs in body order)."""

    nq: int
    nv: int
    nu: int
    ns: int
    jnt_qposadr: list[int]
    jnt_dofadr: list[int]
    dof_body: list[int]
    dof_jnt: list[int]
    body_joints: list[list[int]]


def layout(desc: dict) -> Layout:
    nq = nv = 0
    qa, da, dof_body, dof_jnt = [], [], [], []
    body_joints: list[list[int]] = [[] for _ in desc["bodies"]]
    for j, jn in enumerate(desc["joints"]):
        qa.append(nq)
        da.append(nv)
        n_q, n_v = (7, 6) if jn["type"] == "free" else (1, 1)
        dof_body += [jn["body"]] * n_v
        dof_jnt += [j] * n_v
        body_joints[jn["body"]].append(j)
        nq += n_q
        nv += n_v
    return Layout(nq, nv, len(desc["actuators"]), desc["nsensordata"], qa, da, dof_body, dof_jnt, body_joints)


def qpos0(desc: dict) -> np.ndarray:
    lay = layout(desc)
    q = np.zeros(lay.nq)
    for j, jn in enumerate(desc["joints"]):
        if jn["type"] == "free":
            b = desc["bodies"][jn["body"]]
            q[lay.jnt_qposadr[j] : lay.jnt_qposadr[j] + 7] = list(b["pos"]) + list(b["quat"])
    return q


def _kinematics(desc: dict, q: np.ndarray):
    """Body poses, inertial frames and per-dof motion axes (angular, linear-at-origin) in world coordinates."""
    lay = layout(desc)
    nb = len(desc["bodies"])
    xpos = np.zeros((nb, 3))
    xquat = np.tile([1.0, 0, 0, 0], (nb, 1))
    S = np.zeros((lay.nv, 6))
    for b in range(1, nb):
        body = desc["bodies"][b]
        p = body["parent"]
        joints = lay.body_joints[b]
        if len(joints) == 1 and desc["joints"][joints[0]]["type"] == "free":
            j = joints[0]
            qa, da = lay.jnt_qposadr[j], lay.jnt_dofadr[j]
            pos, quat = q[qa : qa + 3].copy(), q[qa + 3 : qa + 7] / np.linalg.norm(q[qa + 3 : qa + 7])
            R = quat_to_mat(quat)
            for k in range(3):
                S[da + k, 3 + k] = 1.0
                S[da + 3 + k, :3] = R[:, k]
                S[da + 3 + k, 3:] = np.cross(pos, R[:, k])
        else:
            pos = xpos[p] + quat_to_mat(xquat[p]) @ np.array(body["pos"])
            quat = quat_mul(xquat[p], body["quat"])
            for j in joints:
                jn = desc["joints"][j]
                R = quat_to_mat(quat)
                axis = R @ np.array(jn["axis"])
                anchor = pos + R @ np.array(jn["pos"])
                val = q[lay.jnt_qposadr[j]]
                da = lay.jnt_dofadr[j]
                if jn["type"] == "slide":
                    pos = pos + axis * val
                    S[da, 3:] = axis
                else:
                    ql = np.concatenate([[np.cos(val / 2)], np.sin(val / 2) * np.array(jn["axis"])])
                    quat = quat_mul(quat, ql)
                    pos = anchor - quat_to_mat(quat) @ np.array(jn["pos"])
                    S[da, :3] = axis
                    S[da, 3:] = np.cross(anchor, axis)
        xpos[b], xquat[b] = pos, quat / np.linalg.norm(quat)
    return lay, xpos, xquat, S


def _spatial_inertia(mass: float, com: np.ndarray, Ic: np.ndarray) -> np.ndarray:
    cx = np.array([[0, -com[2], com[1]], [com[2], 0, -com[0]], [-com[1], com[0], 0]])
    I = np.zeros((6, 6))
    I[:3, :3] = Ic + mass * (com @ com * np.eye(3) - np.outer(com, com))
    I[:3, 3:] = mass * cx
    I[3:, :3] = mass * cx.T
    I[3:, 3:] = mass * np.eye(3)
    return I


def mass_matrix(desc: dict, q: np.ndarray) -> tuple[np.ndarray, dict]:
    """Joint-space inertia (CRB sum over bodies, + armature) at configuration q."""
    lay, xpos, xquat, S = _kinematics(desc, q)
    nb = len(desc["bodies"])
    # which dofs move each body: its own and its ancestors'
    body_dofs: list[list[int]] = [[] for _ in range(nb)]
    for b in range(1, nb):
        own = [d for d in range(lay.nv) if lay.dof_body[d] == b]
        body_dofs[b] = body_dofs[desc["bodies"][b]["parent"]] + own
    M = np.zeros((lay.nv, lay.nv))
    coms = np.zeros((nb, 3))
    for b in range(1, nb):
        body = desc["bodies"][b]
        R = quat_to_mat(xquat[b])
        com = xpos[b] + R @ np.array(body["ipos"])
        coms[b] = com
        if body["mass"] <= 0:
            continue
        Ri = R @ quat_to_mat(body["iquat"])
        I6 = _spatial_inertia(body["mass"], com, Ri @ np.diag(body["inertia"]) @ Ri.T)
        Sb = S[body_dofs[b]]
        M[np.ix_(body_dofs[b], body_dofs[b])] += Sb @ I6 @ Sb.T
    for d in range(lay.nv):
        M[d, d] += desc["joints"][lay.dof_jnt[d]]["armature"]
    return M, dict(layout=lay, xpos=xpos, xquat=xquat, S=S, body_dofs=body_dofs, coms=coms)


def inverse_weights(desc: dict) -> tuple[np.ndarray, np.ndarray]:
    """(dof_invweight0 (nv,), body_invweight0 (nbody,2)) at qpos0 -- MuJoCo's per-dof / per-body inverse inertia
    measures that scale every constraint regulariser R = (1-d)/d * diagApprox."""
    M, aux = mass_matrix(desc, qpos0(desc))
    lay, S = aux["layout"], aux["S"]
    Minv = np.linalg.inv(M)
    dofw = np.diag(Minv).copy()
    for j, jn in enumerate(desc["joints"]):
        if jn["type"] == "free":
            da = lay.jnt_dofadr[j]
            dofw[da : da + 3] = dofw[da : da + 3].mean()
            dofw[da + 3 : da + 6] = dofw[da + 3 : da + 6].mean()
    nb = len(desc["bodies"])
    bodyw = np.zeros((nb, 2))
    for b in range(1, nb):
        dofs = aux["body_dofs"][b]
        if not dofs:
            continue
        Sb = S[dofs]
        Jr = Sb[:, :3].T  # angular velocity Jacobian
        Jp = np.cross(Sb[:, :3], aux["coms"][b]).T + Sb[:, 3:].T  # velocity of the centre of mass
        Mi = Minv[np.ix_(dofs, dofs)]
        bodyw[b] = (np.trace(Jp @ Mi @ Jp.T) / 3, np.trace(Jr @ Mi @ Jr.T) / 3)
    return dofw, bodyw


def solref_to_kb(solref, solimp, timestep: float) -> tuple[float, float]:
    """(K, B) of the reference acceleration aref = -B*vel - K*imp*pos (MuJoCo solref semantics, refsafe clamp)."""
    dmax = min(0.9999, max(0.0001, solimp[1]))
    if solref[0] > 0:
        tc = max(solref[0], 2 * timestep)
        return 1 / max(MINVAL, dmax * dmax * tc * tc * solref[1] * solref[1]), 2 / max(MINVAL, dmax * tc)
    return -solref[0] / max(MINVAL, dmax * dmax), -solref[1] / max(MINVAL, dmax)


def clamp_solimp(solimp) -> list[float]:
    return [min(0.9999, max(0.0001, solimp[0])), min(0.9999, max(0.0001, solimp[1])), max(0.0, solimp[2]),
            min(0.9999, max(0.0001, solimp[3])), max(1.0, solimp[4])]


def actuator_ctrlrange(desc: dict) -> np.ndarray:
    """(nu, 2) control bounds, +-inf where the actuator is not ctrl-limited (judo/tasks/base.py:98-103)."""
    out = np.zeros((len(desc["actuators"]), 2))
    for i, a in enumerate(desc["actuators"]):
        out[i] = a["ctrlrange"] if a["ctrlrange"] is not None else (-np.inf, np.inf)
    return out


# ----------------------------------------------------------------------------------------- blob packing
def _pack(kind: int, lay: Layout, ntaskparam: int, floats, ints) -> bytes:
    f = np.asarray(floats, dtype=np.float32)
    i = np.asarray(ints, dtype=np.int32)
    head = struct.pack("<16I", BLOB_MAGIC, 1, kind, lay.nq, lay.nv, lay.nu, lay.ns, ntaskparam, f.size, i.size, 0, 0, 0, 0, 0, 0)
    return head + f.tobytes() + i.tobytes()


def _pack_cartpole(desc: dict) -> bytes:
    lay = layout(desc)
    o = desc["option"]
    cart, pole = desc["bodies"][1], desc["bodies"][2]
    jx, jth = desc["joints"]
    act = desc["actuators"][0]
    dofw, _ = inverse_weights(desc)
    K, B = solref_to_kb(jx["solreflimit"], jx["solimplimit"], o["timestep"])
    site_tip = next(s for s in desc["sites"] if s["name"] == "trace_pole")
    P = [
        o["timestep"], -o["gravity"][2], cart["mass"], pole["mass"], pole["ipos"][2], pole["inertia"][0], jx["damping"], jth["damping"],
        act["kp"], act["kv"], *(act["ctrlrange"] or (0, 0)), float(act["ctrlrange"] is not None),
        *(act["forcerange"] or (0, 0)), float(act["forcerange"] is not None),
        *(jx["range"] or (0, 0)), float(jx["range"] is not None), K, B, *clamp_solimp(jx["solimplimit"]), dofw[0], site_tip["pos"][2],
    ]
    return _pack(TASK_KIND["cartpole"], lay, 6, P, [])


def _pack_cylinder(desc: dict) -> bytes:
    lay = layout(desc)
    o = desc["option"]
    pusher, cart = desc["bodies"][2], desc["bodies"][3]
    jp, jc = desc["joints"][0], desc["joints"][2]
    act = desc["actuators"][0]
    gp = next(g for g in desc["geoms"] if g["name"] == "pusher")
    gc = next(g for g in desc["geoms"] if g["name"] == "cart")
    _, bodyw = inverse_weights(desc)
    solref = [0.5 * (a + b) for a, b in zip(gp["solref"], gc["solref"])]
    solimp = [0.5 * (a + b) for a, b in zip(gp["solimp"], gc["solimp"])]
    K, B = solref_to_kb(solref, solimp, o["timestep"])
    mu = max(MINMU, max(gp["friction"][0], gc["friction"][0]))
    margin = max(gp["margin"], gc["margin"]) - max(gp["gap"], gc["gap"])
    site = next(s for s in desc["sites"] if s["name"] == "pusher_site")
    P = [
        o["timestep"], pusher["mass"], cart["mass"], jp["damping"], jc["damping"], act["kp"], act["kv"],
        *(act["ctrlrange"] or (0, 0)), float(act["ctrlrange"] is not None), *(act["forcerange"] or (0, 0)), float(act["forcerange"] is not None),
        gp["size"][0] + gc["size"][0], K, B, *clamp_solimp(solimp), bodyw[2][0] + bodyw[3][0], mu, site["pos"][2], margin,
    ]
    return _pack(TASK_KIND["cylinder_push"], lay, 6, P, [])


def pack_model(desc: dict) -> bytes:
    task = desc.get("family", desc["task"])
    if task == "cartpole":
        return _pack_cartpole(desc)
    if task == "cylinder_push":
        return _pack_cylinder(desc)
    from judo_amd.engine_model import pack_engine_model  # articulated-body engine (leap_cube, fr3_pick)

    return pack_engine_model(desc, pair_tables=bool(desc.get("pair_tables", True)))  # ("pair_tables": false in a description: the leap image without them, every hand pair tested)


# ----------------------------------------------------------------------------------------- randomised physics
def _scale_named(items: list[dict], factors: dict | None, what: str, apply) -> None:
    if not factors:
        return
    names = {it["name"] for it in items}
    for name, factor in factors.items():
        if name is not None and name not in names:
            raise ValueError(f"scaled_description: no {what} named {name!r} (known: {sorted(names)})")
        for it in items:
            if name is None or it["name"] == name:
                apply(it, float(factor))


def scaled_description(desc: dict, *, body_mass: dict | None = None, geom_friction: dict | None = None, actuator_kp: dict | None = None) -> dict:
    """A deep copy of `desc` with perturbed physics: the named bodies' mass and inertia scaled together (the same body, denser), the named geoms' sliding friction
    scaled, the named actuators' `kp` scaled.  Each argument maps a name to a factor; the key `None` means every body / geom / actuator (named keys apply on top of it,
    in the dict's order).  Unknown names raise ValueError; `desc` itself is not touched.

    Nothing else in the description moves, so what changes in the packed image (`pack_model`) is words of its float section alone -- masses, inertias and the inverse
    weights derived from them, friction coefficients, gains -- while the header and the int section (topology, pair lists, lane lists) stay byte for byte: such images
    can share one batched launch (`device.GpuModelSet`, `ControllerFleet`, `make_controller_fleet(..., descriptions=...)`)."""
    out = copy.deepcopy(desc)

    def mass(b: dict, f: float) -> None:
        b["mass"] = b["mass"] * f
        b["inertia"] = [v * f for v in b["inertia"]]

    def friction(g: dict, f: float) -> None:
        g["friction"] = [g["friction"][0] * f] + list(g["friction"][1:])

    def kp(a: dict, f: float) -> None:
        a["kp"] = a["kp"] * f

    _scale_named(out["bodies"], body_mass, "body", mass)
    _scale_named(out["geoms"], geom_friction, "geom", friction)
    _scale_named(out["actuators"], actuator_kp, "actuator", kp)
    return out


def image_sections(blob: bytes) -> tuple[bytes, bytes, bytes]:
    """(header, float section, int section) of a packed image (`pack_model`; the layout of `_pack`): 64 header bytes, then `nfloat` fp32, then `nint` int32."""
    blob = bytes(blob)
    if len(blob) < 64:
        raise ValueError(f"image_sections: {len(blob)} bytes are no model image (the header alone has 64)")
    head = struct.unpack("<16I", blob[:64])
    if head[0] != BLOB_MAGIC:
        raise ValueError(f"image_sections: bad magic {head[0]:08x}")
    nf, ni = head[8], head[9]
    if len(blob) != 64 + 4 * (nf + ni):
        raise ValueError(f"image_sections: {len(blob)} bytes, the header announces {64 + 4 * (nf + ni)}")
    return blob[:64], blob[64 : 64 + 4 * nf], blob[64 + 4 * nf :]
