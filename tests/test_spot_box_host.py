"""spot_box / spot_box_push on the host: the derived model description, its tree image (the object section), jh_tree_create's checks of that section, and the task's
reward and configuration against the reference (tests/golden/spot_box_push.npz and spot_box_push_configs.json, written by tools/gen_golden_spot_box.py)."""

import ctypes
import json
import os

import numpy as np
import pytest

from tests.conftest import GOLDEN, ROOT


def test_spot_box_description():
    """judo/models/xml/spot_box/robot.xml derived from spot.json: 33 / 31 dims, 39 sensor floats, the box body / free joint / geom / site, MuJoCo's pair set."""
    from judo_amd import models
    from oracle import oracle as O

    d = models.load_description("spot_box")
    lay = models.layout(d)
    assert (lay.nq, lay.nv, lay.nu, lay.ns) == (33, 31, 19, 39) and d["nsensordata"] == 39 and d["family"] == "spot"
    bi = next(i for i, b in enumerate(d["bodies"]) if b["name"] == "box_body")
    b = d["bodies"][bi]
    assert b["parent"] == 0 and b["mass"] == 1.5 and b["inertia"] == [0.1445] * 3 and b["ipos"] == [0.0] * 3 and b["pos"] == [2.0, 0.0, 0.254]
    j = d["joints"][-1]
    assert (j["name"], j["type"], j["body"]) == ("box_joint", "free", bi) and lay.jnt_qposadr[-1] == 26 and lay.jnt_dofadr[-1] == 25
    g = next(g for g in d["geoms"] if g["name"] == "box_collision")
    robot = d["geoms"][0]
    assert g["type"] == "box" and g["size"] == [0.254] * 3 and g["priority"] == 4 and g["body"] == bi
    assert (g["friction"], g["solref"], g["solimp"], g["condim"]) == (robot["friction"], robot["solref"], robot["solimp"], robot["condim"])
    site = next(s for s in d["sites"] if s["name"] == "site_object")
    assert site["body"] == bi and site["pos"] == [0.0, 0.0, 0.0]
    assert [s["name"] for s in d["sensors"]] == ["sensor_body", "body_x_axis", "object_x_axis", "object_y_axis", "object_z_axis", "trace_fngr_site", "gripper_x_axis",
                                                 "gripper_y_axis", "finger_x_axis", "fl_pos", "fr_pos", "hl_pos", "hr_pos"]
    assert all(s.get("reftype") is None and s["objtype"] == "site" for s in d["sensors"]) and [s["adr"] for s in d["sensors"]] == list(range(0, 39, 3))
    assert d["bodies"][1]["pos"] == [0.0, 0.0, 0.52]
    # the robot's own description is untouched: spot.json's bodies, joints, geoms are spot_box's minus the box
    spot = models.load_description("spot")
    assert [x["name"] for x in d["geoms"] if x["name"] != "box_collision"] == [x["name"] for x in spot["geoms"]] and d["joints"][:-1] == spot["joints"]
    # the inverse weights of the robot do not depend on where it stands (0.52 vs 0.7)
    w_box, _ = models.inverse_weights(d)
    w_spot, _ = models.inverse_weights(spot)
    np.testing.assert_allclose(w_box[:25], w_spot, rtol=1e-12)
    pairs = O.collision_pairs(d, "all")
    gi = d["geoms"].index(g)
    assert len(pairs) == 342 and sum(gi in p for p in pairs) == 28


def test_spot_box_description_matches_the_mjcf_transcription():
    """tools/compile_mjcf.py transcribes judo/models/xml/spot_box/robot.xml to the same description (a cross-check; only where the reference checkout is present)."""
    import importlib.util

    spec = importlib.util.spec_from_file_location("compile_mjcf", os.path.join(ROOT, "tools", "compile_mjcf.py"))
    cm = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cm)
    if not os.path.exists(os.path.join(cm.REF_XML, "spot_box", "robot.xml")):
        pytest.skip("the reference MJCF is not on this machine")
    from judo_amd import models

    m = cm.transcribe_spot_box()
    d = models.load_description("spot_box")
    for k in ("option", "bodies", "joints", "geoms", "sites", "actuators", "sensors", "excludes", "equalities", "nsensordata"):
        assert json.dumps(m[k], sort_keys=True) == json.dumps(d[k], sort_keys=True), k


def test_spot_box_tree_image():
    """The object section behind everything else: the spot image keeps its layout (I[8:11] = 0), spot_box's carries the box's body record, its plane-mixed geom record
    and the 27 robot-box pairs."""
    from judo_amd import models
    from judo_amd.tree_model import TG_F, TH_F, TH_I, TD_F, TD_I, TG_I, TO_F, TO_I, TS_F, TS_I, pack_tree_blob, pack_tree_model, tree_structure

    Fs, Is = pack_tree_model(models.load_description("spot"))
    assert (Fs.size, Is.size) == (TH_F + 19 * TD_F + 27 * TG_F + 16 * TS_F, TH_I + 19 * TD_I + 27 * TG_I + 16 * TS_I + 287) and not Is[8:16].any() and not Fs[30:32].any()
    d = models.load_description("spot_box")
    st = tree_structure(d)
    assert len(st["hinges"]) == 19 and st["objects"] == [next(i for i, b in enumerate(d["bodies"]) if b["name"] == "box_body")]
    F, I = pack_tree_model(d)
    nj, ng, nq, nv, ns, nsd, npair, opair, nobj, oof, ooi = (int(v) for v in I[:11])
    assert (nj, ng, nq, nv, ns, nsd, npair, nobj) == (19, 27, 33, 31, 13, 39, 287, 1)
    assert oof == TH_F + nj * TD_F + ng * TG_F + ns * TS_F and F.size == oof + TO_F
    assert ooi == opair + npair and I.size == ooi + TO_I + 27
    assert np.array_equal(I[: TH_I + nj * TD_I + ng * TG_I][16:], Is[16: TH_I + nj * TD_I + ng * TG_I])   # joints and robot geoms as in spot's image
    ob = F[oof: oof + TO_F]
    assert ob[0] == np.float32(1.5) and np.allclose(ob[13:16], 0.1445) and np.allclose(ob[4:13], np.eye(3).ravel()) and not ob[1:4].any()
    _, bodyw = models.inverse_weights(d)
    assert np.allclose(ob[16:18], bodyw[st["objects"][0]])
    g = ob[20: 20 + TG_F]
    assert np.allclose(g[0:3], 0.254) and abs(g[15] - 0.7) < 1e-7 and abs(g[25] - 0.15) < 1e-7   # the plane's friction wins (priority 5 > 4); the box's own for robot pairs
    assert abs(g[24] - np.sqrt(3) * 0.254) < 1e-6 and abs(g[23] - bodyw[st["objects"][0]][0]) < 1e-6
    assert list(I[ooi: ooi + TO_I]) == [6, 27, 0, 0] and list(I[ooi + TO_I:]) == list(range(27))
    # sensors on the box's site: owner -3; the world-fixed sites of spot are gone
    srec = I[TH_I + nj * TD_I + ng * TG_I: opair].reshape(ns, TS_I)
    assert list(srec[2:5, 1]) == [-3, -3, -3] and list(srec[2:5, 0]) == [1, 2, 3] and not srec[:, 3].any()
    blob = pack_tree_blob(d)
    assert len(blob) == 16 + 4 * (F.size + I.size)
    # two objects, a cylinder: refused by the packer
    d2 = models.load_description("spot_box")
    d2["bodies"].append(dict(d2["bodies"][st["objects"][0]], name="box2"))
    d2["joints"].append(dict(d2["joints"][-1], name="box2_joint", body=len(d2["bodies"]) - 1))
    with pytest.raises(NotImplementedError):
        pack_tree_model(d2)
    d3 = models.load_description("spot_box")
    next(g for g in d3["geoms"] if g["name"] == "box_collision")["type"] = "cylinder"
    with pytest.raises(NotImplementedError):
        pack_tree_model(d3)


def test_tree_create_rejects_object_sections_outside_the_kernel():
    """jh_tree_create checks the object section before it touches the device: a cylinder object, a second object, a centre of mass off the origin."""
    from judo_amd import _lib, models
    from judo_amd.tree_model import TO_F, pack_tree_blob

    L = _lib.lib()
    L.jh_last_error.restype = ctypes.c_char_p
    blob = pack_tree_blob(models.load_description("spot_box"))
    hd = np.frombuffer(blob[:16], dtype=np.uint32)
    nf = int(hd[1])
    F = np.frombuffer(blob[16: 16 + 4 * nf], dtype=np.float32).copy()
    I = np.frombuffer(blob[16 + 4 * nf:], dtype=np.int32).copy()

    def create(F, I):
        b = hd.tobytes() + F.tobytes() + I.tobytes()
        buf = (ctypes.c_char * len(b)).from_buffer_copy(b)
        h = ctypes.c_void_p()
        rc = L.jh_tree_create(ctypes.cast(buf, ctypes.c_void_p), len(b), ctypes.byref(h))
        return rc, (L.jh_last_error() or b"").decode()

    cyl = I.copy()
    cyl[int(I[10])] = 5   # the object's geom a cylinder
    rc, msg = create(F, cyl)
    assert rc < 0 and "box" in msg
    two = I.copy()
    two[8] = 2            # a second object
    rc, msg = create(F, two)
    assert rc < 0 and "at most one free object" in msg
    off = F.copy()
    off[int(I[9]) + 3] = 0.05   # centre of mass off the body origin
    rc, msg = create(off, I)
    assert rc < 0 and "centre of mass" in msg
    dims = I.copy()
    dims[2] = 26          # an object section on an image that claims the robot's dims only
    rc, msg = create(F, dims)
    assert rc < 0 and "free box" in msg
    assert TO_F == 48


def test_spot_box_push_reward_matches_reference():
    """SpotBoxPush.reward (spot_box_push.py:63-115) on the reference's recorded rollouts: numpy and torch, the default config and one with every weight changed.
    The rollouts trip the fall penalty (incl. the threshold itself) and the orientation count (incl. y . z exactly at the threshold)."""
    import torch

    from judo_amd.spot_tasks import SpotBoxPush

    g = np.load(os.path.join(GOLDEN, "spot_box_push.npz"))
    t = SpotBoxPush()
    assert (t.body_pose_idx, t.object_pose_idx, t.object_y_axis_idx, t.gripper_pos_idx, t.nq, t.nv, t.nsensordata, t.nu) == (0, 26, 9, 15, 33, 31, 39, 10)
    r = t.reward(g["states"], g["sensors"], g["controls"])
    np.testing.assert_allclose(r, g["reward"], rtol=1e-13)
    assert (r < -2000).sum() == 2 and np.abs(np.diff(g["reward"])).max() > 10
    rt = t.reward(torch.as_tensor(g["states"]), torch.as_tensor(g["sensors"]), torch.as_tensor(g["controls"]))
    np.testing.assert_allclose(rt.numpy(), g["reward"], rtol=1e-12)
    c = g["cfg2"]
    t.config.goal_position = c[0:3]
    t.config.w_goal, t.config.w_orientation, t.config.w_torso_proximity, t.config.w_gripper_proximity = c[3:7]
    t.config.orientation_threshold, t.config.fall_penalty, t.config.w_controls, t.config.spot_fallen_threshold = c[7:11]
    np.testing.assert_allclose(t.reward(g["states"], g["sensors"], g["controls"]), g["reward_cfg2"], rtol=1e-13)
    rt = t.reward(torch.as_tensor(g["states"]), torch.as_tensor(g["sensors"]), torch.as_tensor(g["controls"]))
    np.testing.assert_allclose(rt.numpy(), g["reward_cfg2"], rtol=1e-12)


def test_spot_box_push_task_and_overrides_match_reference():
    """Registration, the task's config defaults, the reset pose's layout and the shipped optimizer / controller overrides for spot_box_push."""
    from judo_amd.config import ControllerConfig
    from judo_amd.optimizers import CrossEntropyMethodConfig, MPPIConfig, PredictiveSamplingConfig
    from judo_amd.spot_tasks import ARM_UNSTOWED_POS, LEGS_STANDING_POS, SpotBoxPush, SpotBoxPushConfig
    from judo_amd.tasks import get_registered_tasks

    g = json.load(open(os.path.join(GOLDEN, "spot_box_push_configs.json")))
    assert get_registered_tasks()["spot_box_push"][:2] == (SpotBoxPush, SpotBoxPushConfig)
    assert {k: (v.tolist() if hasattr(v, "tolist") else v) for k, v in vars(SpotBoxPushConfig()).items()} == g["task_defaults"]
    for nm, cls in (("mppi", MPPIConfig), ("cem", CrossEntropyMethodConfig), ("ps", PredictiveSamplingConfig)):
        c = cls()
        c.set_override("spot_box_push")
        assert {k: getattr(c, k) for k in g["optimizer"][nm]} == g["optimizer"][nm]
    c = ControllerConfig()
    c.set_override("spot_box_push")
    assert vars(c) == g["controller"]
    t = SpotBoxPush()
    assert t.use_arm and not t.use_legs and t.model_name == "spot_box" and t.uses_locomotion_policy
    np.random.seed(3)
    poses = np.stack([t.reset_pose for _ in range(200)])
    assert poses.shape == (200, 33) and np.allclose(poses[:, 2], 0.52) and np.allclose(poses[:, 7:19], LEGS_STANDING_POS) and np.allclose(poses[:, 19:26], ARM_UNSTOWED_POS)
    assert np.allclose(poses[:, 28], 0.254) and np.allclose(poses[:, 29:33], [1, 0, 0, 0])
    rad = np.linalg.norm(poses[:, 26:28], axis=1)
    assert rad.max() > 2.5 and rad.min() < 1.0   # radius 1..2 plus randn(2): reaches beyond the ring on both sides
    assert t.data.qpos.shape == (33,) and t.data.qvel.shape == (31,)
