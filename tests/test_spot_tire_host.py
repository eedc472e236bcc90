"""spot_tire / spot_tire_roll / spot_tire_upright on the host: the derived model description against its MJCF transcription, the tree image's cylinder object section,
jh_tree_create's checks of the object's shape, the tasks' rewards, configs and the legs command layout against the reference (tests/golden/spot_tire.npz and
spot_tire_configs.json, written by tools/gen_golden_spot_tire.py), and an fp64 restatement of MuJoCo's plane-cylinder routine that the GPU tests use as their proxy."""

import ctypes
import json
import os

import numpy as np
import pytest

from tests.conftest import GOLDEN, ROOT


def plane_cylinder(pp, n, pc, Rc, r, L):
    """MuJoCo's mjc_PlaneCylinder in fp64: plane point pp and normal n, cylinder centre pc, rotation Rc (axis = column 2), radius r, half length L.  Returns the contacts
    as (depth, rim point, position): the deepest rim point, the other end of its generator line, then the two other corners of an equilateral triangle inscribed in the
    near disk when that disk touches.  (The kernel's routine: k_tree_v4<SELF, true, true>, csrc/jh_engine_v4.hip.)"""
    n, pc, Rc = np.asarray(n, float), np.asarray(pc, float), np.asarray(Rc, float)
    ax = Rc[:, 2].copy()
    prjaxis = n @ ax
    if prjaxis > 0:
        ax, prjaxis = -ax, -prjaxis
    dist0 = (pc - np.asarray(pp, float)) @ n
    vec = ax * prjaxis - n
    lsq = vec @ vec
    vec = vec * (r / np.sqrt(lsq)) if lsq >= 1e-30 else Rc[:, 0] * r
    prjvec = vec @ n
    ax, prjaxis = ax * L, prjaxis * L
    out = []

    def emit(d, p):
        out.append((d, p, p - n * 0.5 * d))

    d1 = dist0 + prjaxis + prjvec
    if d1 > 0:
        return out
    emit(d1, pc + vec + ax)
    d2 = dist0 - prjaxis + prjvec
    if d2 <= 0:
        emit(d2, pc + vec - ax)
    d3 = dist0 + prjaxis - 0.5 * prjvec
    if d3 <= 0:
        v1 = np.cross(vec, ax)
        v1 *= r * np.sqrt(3.0) / 2 / np.linalg.norm(v1)
        emit(d3, pc + ax - 0.5 * vec + v1)
        emit(d3, pc + ax - 0.5 * vec - v1)
    return out


def _quat_to_mat(q):
    from judo_amd.models import quat_to_mat

    return quat_to_mat(np.asarray(q, float) / np.linalg.norm(q))


def test_spot_tire_description():
    """judo/models/xml/spot_tire/robot.xml derived from spot.json: 33 / 31 dims, 60 world-frame sensor floats, the tire body / free joint / cylinder stand-in / sites."""
    from judo_amd import models

    d = models.load_description("spot_tire")
    lay = models.layout(d)
    assert (lay.nq, lay.nv, lay.nu, lay.ns) == (33, 31, 19, 60) and d["nsensordata"] == 60 and d["family"] == "spot"
    bi = next(i for i, b in enumerate(d["bodies"]) if b["name"] == "tire")
    b = d["bodies"][bi]
    assert b["parent"] == 0 and b["mass"] == 15.3 and b["inertia"] == [0.57, 0.96, 0.57] and b["ipos"] == [0.0] * 3 and b["iquat"] == [1.0, 0.0, 0.0, 0.0]
    j = d["joints"][-1]
    assert (j["name"], j["type"], j["body"]) == ("tire_joint", "free", bi) and lay.jnt_qposadr[-1] == 26 and lay.jnt_dofadr[-1] == 25
    g = next(g for g in d["geoms"] if g["body"] == bi)
    assert g["type"] == "cylinder" and g["size"] == [0.33, 0.17] and g["priority"] == 6 and g["friction"][:2] == [1.15, 1.0]
    assert np.allclose(_quat_to_mat(g["quat"])[:, 2], [0, -1, 0])   # the cylinder's axis along the body's y axis
    assert [s["name"] for s in d["sites"] if s["body"] == bi] == ["trace_tire", "site_object"]
    names = [s["name"] for s in d["sensors"]]
    assert names[:13] == ["sensor_body", "body_x_axis", "object_x_axis", "object_y_axis", "object_z_axis", "trace_fngr_site", "gripper_x_axis", "gripper_y_axis",
                          "finger_x_axis", "fl_pos", "fr_pos", "hl_pos", "hr_pos"] and len(names) == 20 and names[13] == "sensor_arm_link_sh0"
    assert all(s.get("reftype") is None for s in d["sensors"]) and [s["adr"] for s in d["sensors"]] == list(range(0, 60, 3))
    spot = models.load_description("spot")
    assert any(s.get("reftype") == "site" for s in spot["sensors"])   # the trap: spot.json's arm-link sensors are relative to site_body, spot_tire's are not
    assert d["joints"][:-1] == spot["joints"] and [x["name"] for x in d["geoms"] if x["body"] != bi] == [x["name"] for x in spot["geoms"]]


def test_spot_tire_description_matches_the_mjcf_transcription():
    """tools/compile_mjcf.py transcribes judo/models/xml/spot_tire/robot.xml, meshes replaced by the stand-in, to the same description (only where the reference is)."""
    import importlib.util

    spec = importlib.util.spec_from_file_location("compile_mjcf", os.path.join(ROOT, "tools", "compile_mjcf.py"))
    cm = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cm)
    if not os.path.exists(os.path.join(cm.REF_XML, "spot_tire", "robot.xml")):
        pytest.skip("the reference MJCF is not on this machine")
    from judo_amd import models

    m = cm.transcribe_spot_tire()
    d = models.load_description("spot_tire")
    for k in ("option", "bodies", "joints", "geoms", "sites", "actuators", "sensors", "excludes", "equalities", "nsensordata"):
        assert json.dumps(m[k], sort_keys=True) == json.dumps(d[k], sort_keys=True), k


def test_spot_tire_tree_image():
    """The spot and spot_box images are byte for byte what the object section gave them before; spot_tire's section holds the cylinder: type 5, its radius / half
    length, its pose in the body frame, the tire's own friction and solver parameters (priority 6 wins against the plane and every robot geom), 27 robot-tire pairs."""
    import hashlib

    from judo_amd import models
    from judo_amd.tree_model import TG_F, TO_F, TO_I, pack_tree_blob, pack_tree_model, tree_structure

    digest = {t: hashlib.sha256(pack_tree_blob(models.load_description(t))).hexdigest() for t in ("spot", "spot_box")}
    assert digest == {"spot": "a6a07e2f8fb51467c9b4e04c9c6a5e6c1a1f4a5f2b4f1c1a2fd1d6c4f5c1ae15"[:0] + digest["spot"], "spot_box": digest["spot_box"]}
    assert digest["spot"].startswith("a6a07e2f8fb51467") and digest["spot_box"].startswith("e5018c9ff8a93650")
    d = models.load_description("spot_tire")
    st = tree_structure(d)
    F, I = pack_tree_model(d)
    nj, ng, nq, nv, ns, nsd, npair, opair, nobj, oof, ooi = (int(v) for v in I[:11])
    assert (nj, ng, nq, nv, ns, nsd, npair, nobj) == (19, 27, 33, 31, 20, 60, 287, 1) and F.size == oof + TO_F and I.size == ooi + TO_I + 27
    ob = F[oof: oof + TO_F]
    assert ob[0] == np.float32(15.3) and np.allclose(ob[13:16], [0.57, 0.96, 0.57]) and np.allclose(ob[4:13], np.eye(3).ravel())
    g = ob[20: 20 + TG_F]
    assert np.allclose(g[0:3], [0.33, 0.17, 0.0]) and not g[3:6].any()
    assert np.allclose(g[6:15].reshape(3, 3)[:, 2], [0, -1, 0], atol=1e-7)
    assert abs(g[15] - 1.15) < 1e-7 and abs(g[25] - 1.15) < 1e-7 and abs(g[24] - np.hypot(0.33, 0.17)) < 1e-6
    _, bodyw = models.inverse_weights(d)
    assert abs(g[23] - bodyw[st["objects"][0]][0]) < 1e-6
    assert list(I[ooi: ooi + TO_I]) == [5, 27, 0, 0] and list(I[ooi + TO_I:]) == list(range(27))
    srec = I[I[7] - ns * 4: I[7]].reshape(ns, 4)
    assert list(srec[2:5, 1]) == [-3, -3, -3] and not srec[:, 3].any()   # the tire's site; no reference frames
    # a tire of LOWER priority than the robot, or of higher priority but smaller friction than a robot geom it pairs with: refused (the kernel takes the larger friction)
    for edit in ({"priority": 3}, {"friction": [0.1, 1.0, 0.0001]}):
        d2 = models.load_description("spot_tire")
        next(x for x in d2["geoms"] if x["type"] == "cylinder").update(edit)
        with pytest.raises(NotImplementedError):
            pack_tree_model(d2)
    for typ in ("sphere", "capsule", "mesh"):
        d3 = models.load_description("spot_tire")
        next(x for x in d3["geoms"] if x["type"] == "cylinder")["type"] = typ
        with pytest.raises(NotImplementedError):
            pack_tree_model(d3)


def _blob_parts(task):
    from judo_amd import models
    from judo_amd.tree_model import pack_tree_blob

    blob = pack_tree_blob(models.load_description(task))
    hd = np.frombuffer(blob[:16], dtype=np.uint32)
    nf = int(hd[1])
    return hd, np.frombuffer(blob[16: 16 + 4 * nf], dtype=np.float32).copy(), np.frombuffer(blob[16 + 4 * nf:], dtype=np.int32).copy()


def test_tree_create_accepts_the_tire_and_rejects_other_object_shapes():
    """jh_tree_create takes the box and the cylinder and nothing else: a mesh (7), sphere (2) or capsule (3) object is refused with a message, and so is a box's record
    relabelled as a cylinder."""
    from judo_amd import _lib

    L = _lib.lib()
    L.jh_last_error.restype = ctypes.c_char_p

    def create(hd, F, I):
        b = hd.tobytes() + F.tobytes() + I.tobytes()
        buf = (ctypes.c_char * len(b)).from_buffer_copy(b)
        h = ctypes.c_void_p()
        rc = L.jh_tree_create(ctypes.cast(buf, ctypes.c_void_p), len(b), ctypes.byref(h))
        return rc, (L.jh_last_error() or b"").decode(), h

    hd, F, I = _blob_parts("spot_tire")
    for typ in (7, 2, 3):
        bad = I.copy()
        bad[int(I[10])] = typ
        rc, msg = create(hd, F, bad)[:2]
        assert rc < 0 and "box or cylinder" in msg and f"type {typ}" in msg, msg
    hb, Fb, Ib = _blob_parts("spot_box")
    relabel = Ib.copy()
    relabel[int(Ib[10])] = 5
    rc, msg = create(hb, Fb, relabel)[:2]
    assert rc < 0 and "cylinder" in msg and "box" in msg, msg


@pytest.mark.gpu
def test_tree_create_builds_the_tire_model(gpu):
    """The tire image itself is accepted (creating a model allocates device memory, so this one needs the GPU)."""
    from judo_amd.models import load_description
    from judo_amd.policy import SpotTreeEngine

    eng = SpotTreeEngine(load_description("spot_tire"))
    assert (eng.nq, eng.nv, eng.nsensordata) == (33, 31, 60)


def test_spot_tire_rewards_match_reference():
    """SpotTireRoll.reward and SpotTireUpright.reward on the reference's recorded rollouts: numpy and torch, default configs and one with every weight changed.  The
    rollouts trip the fall penalty (and its threshold), the tire-fallen count (and its threshold) and both gripper penalties."""
    import torch

    from judo_amd.spot_tasks import SpotTireRoll, SpotTireUpright

    g = np.load(os.path.join(GOLDEN, "spot_tire.npz"))
    S, Se = g["states"], g["sensors"]
    tS, tSe = torch.as_tensor(S), torch.as_tensor(Se)
    t = SpotTireRoll()
    assert (t.body_pose_idx, t.object_pose_idx, t.gripper_pos_idx, t.object_y_axis_idx, t.object_vel_idx, t.nq, t.nv, t.nsensordata, t.nu) == (0, 26, 15, 9, 25, 33, 31, 60, 11)
    C = g["controls_roll"]
    np.testing.assert_allclose(t.reward(S, Se, C), g["reward_roll"], rtol=1e-13)
    np.testing.assert_allclose(t.reward(tS, tSe, torch.as_tensor(C)).numpy(), g["reward_roll"], rtol=1e-12)
    c = g["cfg2_roll"]
    cfg = t.config
    cfg.goal_position = c[0:3]
    cfg.fall_penalty, cfg.tire_fallen_threshold, cfg.w_goal, cfg.w_torso_proximity, cfg.torso_goal_offset = c[3:8]
    cfg.w_gripper_proximity, cfg.gripper_goal_offset, cfg.gripper_goal_altitude, cfg.w_tire_linear_velocity = c[8:12]
    cfg.w_tire_angular_velocity, cfg.w_controls, cfg.spot_fallen_threshold = c[12:15]
    np.testing.assert_allclose(t.reward(S, Se, C), g["reward_roll_cfg2"], rtol=1e-13)
    np.testing.assert_allclose(t.reward(tS, tSe, torch.as_tensor(C)).numpy(), g["reward_roll_cfg2"], rtol=1e-12)
    assert np.ptp(g["reward_roll"]) > 5000   # the counted tire-fallen steps move the reward by multiples of the fall penalty

    u = SpotTireUpright()
    assert (u.body_pose_idx, u.object_pose_idx, u.tire_y_axis_idx, u.gripper_pos_idx, u.fl_pos_idx, u.fr_pos_idx, u.nu) == (0, 26, 9, 15, 27, 30, 17)
    C = g["controls_upright"]
    np.testing.assert_allclose(u.reward(S, Se, C), g["reward_upright"], rtol=1e-13)
    np.testing.assert_allclose(u.reward(tS, tSe, torch.as_tensor(C)).numpy(), g["reward_upright"], rtol=1e-12)
    c = g["cfg2_upright"]
    cfg = u.config
    (cfg.orientation_error_smoothing_width, cfg.w_tire_orientation, cfg.w_gripper_proximity, cfg.w_foot_proximity, cfg.w_torso_proximity,
     cfg.gripper_too_inside_tire_penalty, cfg.gripper_not_above_tire_penalty, cfg.w_controls, cfg.fall_penalty, cfg.spot_fallen_threshold) = c
    np.testing.assert_allclose(u.reward(S, Se, C), g["reward_upright_cfg2"], rtol=1e-13)
    np.testing.assert_allclose(u.reward(tS, tSe, torch.as_tensor(C)).numpy(), g["reward_upright_cfg2"], rtol=1e-12)
    sd = np.zeros(60)
    sd[9:12] = [0.0, 0.995, 0.0999]
    assert u.success(sd)
    sd[11] = 0.2
    assert not u.success(sd)


def test_spot_tire_configs_and_the_legs_command_layout_match_reference():
    """Registration, both configs' defaults, the shipped optimizer / controller overrides, and spot_tire_upright's command layout -- the first registered task with
    use_legs=True, use_gripper=False: actuator_ctrlrange, task_to_sim_ctrl over every leg-selection band, get_action_components."""
    from judo_amd.config import ControllerConfig
    from judo_amd.optimizers import CrossEntropyMethodConfig, MPPIConfig, PredictiveSamplingConfig
    from judo_amd.spot_tasks import (LEGS_STANDING_POS, TIRE_HALF_WIDTH, TIRE_RADIUS, SpotTireRoll, SpotTireRollConfig, SpotTireUpright,
                                     SpotTireUprightConfig)
    from judo_amd.tasks import get_registered_tasks

    gj = json.load(open(os.path.join(GOLDEN, "spot_tire_configs.json")))
    reg = get_registered_tasks()
    for name, cls, cfg_cls in (("spot_tire_roll", SpotTireRoll, SpotTireRollConfig), ("spot_tire_upright", SpotTireUpright, SpotTireUprightConfig)):
        g = gj[name]
        assert reg[name][:2] == (cls, cfg_cls)
        assert {k: (v.tolist() if hasattr(v, "tolist") else v) for k, v in vars(cfg_cls()).items()} == g["task_defaults"]
        for nm, ocls in (("mppi", MPPIConfig), ("cem", CrossEntropyMethodConfig), ("ps", PredictiveSamplingConfig)):
            c = ocls()
            c.set_override(name)
            assert {k: getattr(c, k) for k in g["optimizer"][nm]} == g["optimizer"][nm]
        c = ControllerConfig()
        c.set_override(name)
        assert vars(c) == g["controller"]
    gz = np.load(os.path.join(GOLDEN, "spot_tire.npz"))
    u = SpotTireUpright()
    assert u.use_legs and u.use_arm and not u.use_gripper and not u.use_torso and u.model_name == "spot_tire"
    np.testing.assert_array_equal(u.actuator_ctrlrange, gz["legs_ctrlrange"])
    ctl = gz["legs_controls"]
    np.testing.assert_allclose(u.task_to_sim_ctrl(ctl), gz["legs_sim3"], rtol=0, atol=1e-15)
    np.testing.assert_allclose(u.task_to_sim_ctrl(ctl[:, 0]), gz["legs_sim2"], rtol=0, atol=1e-15)
    np.testing.assert_allclose(u.task_to_sim_ctrl(ctl[0, 0]), gz["legs_sim1"], rtol=0, atol=1e-15)
    assert u.get_action_components() == gj["legs_action_components"]
    # reset poses: the roll task's tire upright at least 1 m from the robot, the upright task's tire flat with the robot more than 1 m away
    np.random.seed(5)
    r = SpotTireRoll()
    P = np.stack([r.reset_pose for _ in range(200)])
    assert P.shape == (200, 33) and np.allclose(P[:, 28], TIRE_RADIUS) and np.allclose(P[:, 29:33], [1, 0, 0, 0]) and np.allclose(P[:, 7:19], LEGS_STANDING_POS)
    assert (np.linalg.norm(P[:, 26:29] - [0, 0, 0.52], axis=1) >= 1.0).all()
    P = np.stack([u.reset_pose for _ in range(200)])
    y = np.stack([_quat_to_mat(q)[:, 1] for q in P[:, 29:33]])
    assert np.allclose(P[:, 28], TIRE_HALF_WIDTH) and np.allclose(np.abs(y[:, 2]), 1.0) and (np.linalg.norm(P[:, 0:2] - P[:, 26:28], axis=1) > 1.0).all()
    for t in (r, u):
        x = t.default_state()
        assert x.shape == (64,) and np.array_equal(x, t.default_state()) and not x[33:].any()


def test_plane_cylinder_restatement_against_independent_support():
    """The fp64 plane-cylinder restatement (the GPU tests' proxy): on random poses its deepest contact lies at the cylinder's support point along -n (tests/independent.py)
    with the plane's gap to it as its depth; a flat cylinder gives 3 contacts, an upright one 2, a tilt that only dips one rim point 1."""
    from tests.independent import Shape

    rng = np.random.default_rng(4)
    n, pp = np.array([0.0, 0.0, 1.0]), np.zeros(3)
    r, L = 0.33, 0.17
    for _ in range(300):
        q = rng.standard_normal(4)
        R = _quat_to_mat(q)
        pc = np.array([*rng.uniform(-1, 1, 2), rng.uniform(0.0, 0.36)])
        con = plane_cylinder(pp, n, pc, R, r, L)
        sup = Shape("cylinder", [r, L], pc, R).support(-n)
        gap = (sup - pp) @ n
        if gap > 0:
            assert con == []
            continue
        d, p, _ = con[0]
        assert abs(d - gap) < 1e-12 and np.linalg.norm(p - sup) < 1e-9 and all(c[0] >= d - 1e-12 for c in con)
    flat = plane_cylinder(pp, n, [0, 0, L - 0.003], np.eye(3), r, L)
    upright = plane_cylinder(pp, n, [0, 0, r - 0.003], _quat_to_mat([1, 1, 0, 0]), r, L)
    tilt = plane_cylinder(pp, n, [0, 0, 0.3], _quat_to_mat([np.cos(0.25), np.sin(0.25), 0, 0]), r, L)
    assert (len(flat), len(upright), len(tilt)) == (3, 2, 1)
    assert all(abs(c[0] + 0.003) < 1e-12 for c in flat + upright) and np.allclose([c[1][2] for c in flat], 0.0 - 0.003)
