"""Device model image for the articulated-body rollout engines (the leap and fr3 kernels, `judo_amd/csrc/jh_engine_v5.hip` and `jh_engine_v6.hip`).

Structure the engine exploits (it holds for leap_cube and fr3_pick): ONE free body (the manipulated cube) plus
articulated "blocks" (serial chains / small trees of hinge or slide joints) hanging off bodies that are welded to
the world.  Consequences used by the kernels:
  * the joint-space inertia is block diagonal: diag(m,m,m,I1,I2,I3) for the free body (its centre of mass sits at
    the body origin) and one small dense block per chain -- no nv x nv factorisation of M is ever needed;
  * static bodies and their collision geoms have constant world poses, folded in here on the host;
  * every contact modelled this round is cube <-> hand geom, so a contact row touches the 6 cube DoF and at most
    one block: the Newton Hessian is an arrow matrix (cube block + per-chain blocks + cube-chain couplings).

The layout of the float (F) and int (I) sections is written down once, in `judo_amd/csrc/jh_image.h`: the table at its top, the constants and slot names that the ones
below repeat (tests/test_image_layout.py holds the two sides to each other), and `struct EngineModel`, whose `init` is `image_offsets` here.
"""

from __future__ import annotations

import collections
import types

import numpy as np

from judo_amd.models import (
    MINMU,
    MINVAL,
    TASK_KIND,
    _pack,
    clamp_solimp,
    inverse_weights,
    layout,
    quat_mul,
    quat_to_mat,
    solref_to_kb,
)

JFREE, JSLIDE, JHINGE = 0, 2, 3
GBOX, GSPHERE, GCAPSULE, GCYLINDER = 6, 2, 3, 5  # (MuJoCo's geom type codes)
GTYPE = {"box": GBOX, "sphere": GSPHERE, "capsule": GCAPSULE, "cylinder": GCYLINDER}
MAX_MOVING, MAX_DOF, MAX_BLOCKS, MAX_BLOCK_DOF, MAX_GEOM, MAX_SITE = 20, 24, 4, 9, 80, 8

# ints per record
BODY_I, GEOM_I, ACT_I, BLOCK_I, SENS_I, EQ_I = 6, 2, 2, 4, 3, 5
# floats per record
BODY_F, DOF_F, ACT_F, GEOM_F, SITE_F, EQ_F, FRAME_F, GP_F = 32, 20, 8, 20, 3, 12, 12, 8
HEADER_I, HEADER_F = 24, 24
LANES, BODY_CODES, BV_F, REF_F, GEN_I = 16, 20, 8, 16, 8  # lane lists; the hand's body codes and floats per bounding volume; reference frames; the generic block's counts
# header ints (jh_image.h has the table): counts, integrator, cone; lane lists (offset, length of a list); generic block (ints, floats); body pairs, bounding
# volumes, number of pairs; reference frames; pair tables; the two words of diagnostic builds
(HI_NM, HI_NBLK, HI_NV, HI_NQ, HI_NU, HI_NG, HI_NSITE, HI_NS, HI_INTEG, HI_CONE, HI_NSENS, HI_LANES, HI_LGM, HI_GI, HI_GF, HI_BP, HI_BS, HI_NBP, HI_REF, HI_PT,
 HI_ABLATE, HI_ABLATE_N) = range(22)
GI_NAG, GI_NPAIR, GI_NEQ, GI_NFRAME, GI_NDIST, GI_NGS = range(6)  # the generic block's own counts
BF_LPOS, BF_LR, BF_AXIS = 0, 3, 28  # body floats: frame in the parent (position, rotation), joint axis
DF_LIMITED, DF_LO, DF_HI = 6, 7, 8  # dof floats: the joint's range
GF_SIZE, GF_POS, GF_R, GF_RBOUND = 0, 3, 6, 15  # geom floats

# Newton termination on the GPU: |grad|_Minv <= tol * |qfrc_smooth|_Minv (or the expected decrease of a step falls below
# tol^2 of the same scale), at most SOLVER_MAX_ITER iterations (MuJoCo: tolerance 1e-8 in fp64, 100 iterations); the exact line search
# stops at |slope| <= SOLVER_LS_TOL * |slope at 0| (MuJoCo's ls_tolerance default is 0.01 too; 1e-3 costs 2.4 % more on fixed plan inputs
# and does not save a single Newton iteration, tools/diag/ab_fixed_inputs.py).
# tol = 1e-5 is where the returned MPPI nominal stops moving with the tolerance on the recorded 40 plan steps of the headline workload
# (profiles/r02_tolerance_sweep.txt: against tol 1e-6 with a 48-contact pool, 25 of the 40 plans pick another winner at 1e-3, 5 at 1e-4, 2 at 1e-5
# and 2 at 1e-6 -- the rest is the 32-contact pool); it costs 2.7 % over 1e-4 (6.86 instead of 6.57 iterations per step).
# 50 iterations instead of round 1's 20: the random-state sweep tools/diag/fuzz_leap.py has states on which the fp64 oracle needs 21-31; on the headline workload the
# higher cap costs nothing measurable (4e-4 solves per step used to stop at 20).
SOLVER_TOL, SOLVER_MAX_ITER, SOLVER_LS_TOL = 1e-5, 50, 1e-2
# diagnostics: (phase, repeats) read only by -DJH_V2_ABLATE builds of the cooperative kernel (tools/diag/time_ablate.py)
ABLATE = (0, 1)


def image_offsets(I) -> types.SimpleNamespace:
    """Where the sections of an image start, from its int section (a list under construction, or an array): `EngineModel::init` of jh_image.h restated, name for name
    -- every run of records starts where the one before it ends -- with the leap family's sections as its `HostImage` names them (zero where the image has none).
    The generic block's entries are there once the block is."""
    slots = (("NM", HI_NM), ("NBLK", HI_NBLK), ("NV", HI_NV), ("NQ", HI_NQ), ("NU", HI_NU), ("NG", HI_NG), ("NSITE", HI_NSITE), ("NS", HI_NS), ("NSENS", HI_NSENS), ("cone", HI_CONE),
             ("oLane", HI_LANES), ("LGM", HI_LGM), ("oBP", HI_BP), ("NBP", HI_NBP), ("oBS", HI_BS), ("oRef", HI_REF), ("oPT", HI_PT))
    o = types.SimpleNamespace(**{name: int(I[slot]) for name, slot in slots})

    def run(start, records):  # (name, ints or floats the records take)
        for name, size in records:
            setattr(o, name, start)
            start += size

    run(HEADER_I, (("oBodyI", o.NM * BODY_I), ("oBlockI", o.NBLK * BLOCK_I), ("oActI", o.NU * ACT_I), ("oGeomI", o.NG * GEOM_I), ("oSiteI", o.NSITE), ("oSensI", 0)))
    run(HEADER_F, (("oBodyF", o.NM * BODY_F), ("oDofF", o.NV * DOF_F), ("oActF", o.NU * ACT_F), ("oGeomF", o.NG * GEOM_F), ("oSiteF", 0)))
    o.oBG = o.oBP + 2 * o.NBP
    gi, gf = int(I[HI_GI]), int(I[HI_GF])
    if gi > 0:
        for name, k in (("NAG", GI_NAG), ("NPAIR", GI_NPAIR), ("NEQ", GI_NEQ), ("NFRAME", GI_NFRAME), ("NDIST", GI_NDIST), ("NGS", GI_NGS)):
            setattr(o, name, int(I[gi + k]))
        run(gi + GEN_I, (("oAGI", o.NAG * GEOM_I), ("oPairI", o.NPAIR * 2), ("oEqI", o.NEQ * EQ_I), ("oFrameI", o.NFRAME), ("oDistI", o.NDIST * 4), ("oSensG", o.NGS * 4), ("oGlist", 0)))
        run(gf, (("oAGF", o.NAG * GEOM_F), ("oGPF", o.NAG * GP_F), ("oEqF", o.NEQ * EQ_F), ("oFrameF", o.NFRAME * FRAME_F), ("oDistF", 0)))
    return o


def blob_sections(blob: bytes) -> tuple[np.ndarray, np.ndarray]:
    """The float and the int section of a packed image."""
    nf = int(np.frombuffer(blob[:64], np.uint32)[8])
    return np.frombuffer(blob[64: 64 + 4 * nf], np.float32), np.frombuffer(blob[64 + 4 * nf:], np.int32)


def _static_world_pose(desc: dict, b: int) -> tuple[np.ndarray, np.ndarray]:
    """World pose of a body whose whole ancestry is joint-free."""
    chain = []
    while b > 0:
        chain.append(b)
        b = desc["bodies"][b]["parent"]
    pos, quat = np.zeros(3), np.array([1.0, 0, 0, 0])
    for bb in reversed(chain):
        body = desc["bodies"][bb]
        pos = pos + quat_to_mat(quat) @ np.array(body["pos"])
        quat = quat_mul(quat, body["quat"])
    return pos, quat / np.linalg.norm(quat)


def engine_structure(desc: dict) -> dict:
    """Classify bodies: static / free / articulated blocks; returns index maps used by the packer and the tests."""
    lay = layout(desc)
    nb = len(desc["bodies"])
    joints_of = lay.body_joints
    is_static = [False] * nb
    is_static[0] = True
    for b in range(1, nb):
        is_static[b] = (len(joints_of[b]) == 0) and is_static[desc["bodies"][b]["parent"]]
    moving = [b for b in range(1, nb) if not is_static[b]]
    for b in moving:
        if len(joints_of[b]) != 1:
            raise NotImplementedError(f"body {desc['bodies'][b]['name']}: the engine needs exactly one joint per moving body")
    free = [b for b in moving if desc["joints"][joints_of[b][0]]["type"] == "free"]
    if len(free) != 1 or moving[0] != free[0]:
        raise NotImplementedError("the engine needs exactly one free body, listed before the articulated bodies")
    fb = desc["bodies"][free[0]]
    if desc["bodies"][fb["parent"]]["parent"] != -1 and fb["parent"] != 0:
        raise NotImplementedError("free body must hang off the world")
    if np.abs(fb["ipos"]).max() > 0 or abs(abs(fb["iquat"][0]) - 1) > 1e-12:
        raise NotImplementedError("free body: centre of mass must be the body origin and the inertia axis-aligned")
    midx = {b: i for i, b in enumerate(moving)}
    # blocks: connected components of articulated bodies (root = body whose parent is static)
    block_of, blocks = {}, []
    for b in moving[1:]:
        p = desc["bodies"][b]["parent"]
        if is_static[p]:
            block_of[b] = len(blocks)
            blocks.append([b])
        else:
            if p not in block_of:
                raise NotImplementedError("articulated body attached to the free body is not supported")
            block_of[b] = block_of[p]
            blocks[block_of[b]].append(b)
    for blk in blocks:
        if blk != list(range(blk[0], blk[0] + len(blk))):
            raise NotImplementedError("bodies of a block must be contiguous (depth-first MJCF order)")
    return dict(layout=lay, is_static=is_static, moving=moving, midx=midx, blocks=blocks, block_of=block_of, free=free[0])


def _mat_to_quat(R: np.ndarray) -> np.ndarray:
    """Rotation matrix -> unit quaternion (w, x, y, z)."""
    t = np.trace(R)
    if t > 0:
        s = np.sqrt(t + 1.0) * 2
        q = np.array([0.25 * s, (R[2, 1] - R[1, 2]) / s, (R[0, 2] - R[2, 0]) / s, (R[1, 0] - R[0, 1]) / s])
    else:
        i = int(np.argmax(np.diag(R)))
        j, k = (i + 1) % 3, (i + 2) % 3
        s = np.sqrt(R[i, i] - R[j, j] - R[k, k] + 1.0) * 2
        q = np.zeros(4)
        q[0] = (R[k, j] - R[j, k]) / s
        q[1 + i] = 0.25 * s
        q[1 + j] = (R[j, i] + R[i, j]) / s
        q[1 + k] = (R[k, i] + R[i, k]) / s
    return q / np.linalg.norm(q)


def fuse_fixed_bodies(desc: dict) -> dict:
    """Merge every joint-less body whose parent moves into that parent (fr3_pick: `hand` is welded to `fr3_link7`).

    MuJoCo keeps such bodies and lets them ride on the parent; the engine wants exactly one joint per moving body, so the
    child's inertia is added to the parent (parallel-axis, re-diagonalised), its children / geoms / sites are re-expressed
    in the parent frame, and sensors that referenced the body frame get an equivalent site.  Geoms remember the body
    they came from (`orig_body`) because contact regularisation and distance sensors are defined per original body."""
    import copy

    d = copy.deepcopy(desc)
    for g in d["geoms"]:
        g.setdefault("orig_body", g["body"])
    lay = layout(d)
    nb = len(d["bodies"])
    static = [True] + [False] * (nb - 1)
    for b in range(1, nb):
        static[b] = (len(lay.body_joints[b]) == 0) and static[d["bodies"][b]["parent"]]
    victims = [b for b in range(1, nb) if len(lay.body_joints[b]) == 0 and not static[b]]
    if not victims:
        return d
    b = victims[0]
    body = d["bodies"][b]
    p = body["parent"]
    par = d["bodies"][p]
    Rb, pb = quat_to_mat(body["quat"]), np.array(body["pos"])
    # inertia merge in the parent frame
    m1, m2 = par["mass"], body["mass"]
    c1, c2 = np.array(par["ipos"]), pb + Rb @ np.array(body["ipos"])
    R1 = quat_to_mat(par["iquat"])
    R2 = Rb @ quat_to_mat(body["iquat"])
    I1, I2 = R1 @ np.diag(par["inertia"]) @ R1.T, R2 @ np.diag(body["inertia"]) @ R2.T
    m = m1 + m2
    c = (m1 * c1 + m2 * c2) / m if m > 0 else c1
    shift = lambda mm, r: mm * (r @ r * np.eye(3) - np.outer(r, r))  # noqa: E731
    I = I1 + shift(m1, c1 - c) + I2 + shift(m2, c2 - c)
    w, V = np.linalg.eigh(I)
    if np.linalg.det(V) < 0:
        V[:, 2] = -V[:, 2]
    par.update(mass=m, ipos=c.tolist(), iquat=_mat_to_quat(V).tolist(), inertia=w.tolist())
    for ch in d["bodies"]:
        if ch.get("parent") == b:
            ch["pos"] = (pb + Rb @ np.array(ch["pos"])).tolist()
            ch["quat"] = quat_mul(body["quat"], ch["quat"]).tolist()
            ch["parent"] = p
    for coll in (d["geoms"], d["sites"]):
        for g in coll:
            if g["body"] == b:
                g["pos"] = (pb + Rb @ np.array(g["pos"])).tolist()
                g["quat"] = quat_mul(body["quat"], g.get("quat", [1, 0, 0, 0])).tolist()
                g["body"] = p
    # sensors on the body frame -> an equivalent site on the parent
    for sn in d["sensors"]:
        if sn["type"] in ("framepos", "framezaxis") and sn.get("objtype") == "body" and sn["obj"] == b:
            d["sites"].append(dict(name=f"{body['name']}_frame", body=p, pos=pb.tolist(), quat=list(body["quat"])))
            sn["objtype"], sn["obj"] = "site", len(d["sites"]) - 1
    # drop body b, renumber
    remap = {i: (i if i < b else i - 1) for i in range(nb) if i != b}
    del d["bodies"][b]
    for ch in d["bodies"]:
        if ch["parent"] >= 0:
            ch["parent"] = remap[ch["parent"]]
    for coll in (d["geoms"], d["sites"], d["joints"]):
        for g in coll:
            g["body"] = remap[g["body"]]
    for sn in d["sensors"]:
        if sn["type"] in ("framepos", "framezaxis", "framequat") and sn.get("objtype") == "body":
            sn["obj"] = remap[sn["obj"]]
    d["excludes"] = [[remap[a], remap[c2]] for a, c2 in d["excludes"] if a != b and c2 != b]
    d.setdefault("fused", []).append(body["name"])
    return fuse_fixed_bodies(d)


def sensor_reference_frames(desc: dict) -> list[float] | None:
    """World pose of the (static) reference frames of `framepos ... reftype=site` / `framequat ... reftype=body` sensors, resolved on the description as
    compiled (before static bodies are fused away): [p_ref(3), R_ref(9), q_ref(4)], or None when no sensor has a reference frame on the engine's models
    (caltech_leap_cube: cube position in the frame of `grasp_site` on the hand mount, cube orientation relative to the mocap goal body at its model pose --
    the pose every rollout thread's MjData starts with, judo/utils/mj_rollout_backend.py:38-43)."""
    weld = lambda b: all(j["body"] != b for j in desc["joints"]) and (desc["bodies"][b]["parent"] < 0 or weld(desc["bodies"][b]["parent"]))  # noqa: E731
    p_ref, R_ref, q_ref, found = np.zeros(3), np.eye(3), np.array([1.0, 0, 0, 0]), False
    for sn in desc["sensors"]:
        if sn["type"] == "framepos" and sn.get("reftype") == "site" and sn.get("objtype") == "body":
            site = desc["sites"][sn["ref"]]
            if not weld(site["body"]):
                raise NotImplementedError("framepos relative to a moving site")
            bp, bq = _static_world_pose(desc, site["body"])
            p_ref = bp + quat_to_mat(bq) @ np.array(site["pos"])
            R_ref = quat_to_mat(quat_mul(bq, site.get("quat", [1, 0, 0, 0])))
            found = True
        elif sn["type"] == "framequat":
            if sn.get("reftype") == "body":
                if not weld(sn["ref"]):
                    raise NotImplementedError("framequat relative to a moving body")
                q_ref = np.array(_static_world_pose(desc, sn["ref"])[1], dtype=np.float64)
            found = True
    return [*p_ref, *R_ref.reshape(-1), *q_ref] if found else None


def generic_pairs(desc: dict, fused: dict, st: dict, cube_only: bool | None = None) -> list[tuple[int, int]]:
    """Candidate box-box / box-sphere pairs for the generic (reference-kernel) contact path, MuJoCo's static filters
    applied on the ORIGINAL bodies: same welded body, parent-child (unless the parent is welded to the world), excludes.
    leap_cube: restricted to pairs that involve the cube (hand self-collision is out of scope this round).
    fr3_pick: the arm links' capsules against static geometry and the free body only (78 pairs, what the default build of k_fr3_v6 collides), unless the description
    carries "self_collision": then every pair the MJCF leaves (190 = oracle.collision_pairs(desc)), the other 112 -- link against link, hand / finger box against link --
    BEHIND the default list, which stays a prefix."""
    arm_pairs = bool(desc.get("self_collision", False))
    bodies = desc["bodies"]
    njnt = [0] * len(bodies)
    for j in desc["joints"]:
        njnt[j["body"]] += 1

    def weld(b):
        while b > 0 and njnt[b] == 0:
            b = bodies[b]["parent"]
        return b

    def weld_parent(b):
        w = weld(b)
        return weld(bodies[w]["parent"]) if w > 0 else 0

    excl = {tuple(sorted(e)) for e in desc["excludes"]}
    geoms = fused["geoms"]
    free_fused = st["free"]
    out, extra = [], []
    for a in range(len(geoms)):
        for b in range(a + 1, len(geoms)):
            ia, ib = a, b
            if geoms[a]["type"] == "capsule" and geoms[b]["type"] == "box":  # (box, capsule) is the order the kernels take, whichever geom the model lists first
                ia, ib = b, a
            ga, gb = geoms[ia], geoms[ib]
            ta, tb = ga["type"], gb["type"]
            round_ = ("sphere", "cylinder")  # (a cylinder is in `geoms` only when the image keeps the fingertips as the MJCF has them: pack_engine_model(fingertips="cylinder"))
            if not ((ta == "box" and tb in ("box", "sphere", "capsule", "cylinder")) or (ta in round_ and tb == "box") or (ta in round_ and tb in round_ and cube_only is False)
                    or (arm_pairs and ta == tb == "capsule")):
                continue  # (sphere-sphere, and cylinder against sphere or cylinder: the fingertips of two fingers; only jh_engine_v5.hip collides the hand with itself)
            ba, bb = ga["orig_body"], gb["orig_body"]
            wa, wb = weld(ba), weld(bb)
            new = ta == "capsule" or (tb == "capsule" and not (wa == 0 or ga["body"] == free_fused))
            if new and not arm_pairs:
                continue  # the arm links' stand-ins meet static geometry and the free body only (oracle/oracle.py::collision_pairs has the reason) in the default image
            if wa == wb or tuple(sorted((ba, bb))) in excl:
                continue
            if (weld_parent(ba) == wb and wb != 0) or (weld_parent(bb) == wa and wa != 0):
                continue
            leap = desc.get("family", desc["task"]) == "leap_cube"
            if (leap if cube_only is None else cube_only) and free_fused not in (ga["body"], gb["body"]):
                continue  # (the one-lane reference kernel and jh_engine_v2.hip model the cube's contacts only; jh_engine_v5.hip adds the hand's own)
            (extra if new else out).append((ia, ib))
    # order by importance for the fixed-capacity contact pools: pairs with the free body first, then pairs against static
    # geometry, pairs between two articulated bodies (e.g. the two fingers' pad stacks) last -- those are the ones dropped on overflow
    def rank(pr):
        ba, bb = geoms[pr[0]]["body"], geoms[pr[1]]["body"]
        if free_fused in (ba, bb):
            return 0
        return 1 if (st["is_static"][ba] or st["is_static"][bb]) else 2
    out.sort(key=rank)  # stable: original order within a class
    return out + extra  # (the self-collision image's own pairs, in model order)


def kernel_stand_ins(desc: dict) -> dict:
    """The description as the leap KERNEL collides it (jh_engine_v5.hip has box and sphere narrow phases only): caltech_leap_cube's fingertip cylinders
    (judo/models/xml/caltech_leap_components/leap_rh.xml:131,175,219,259: r = 14 mm, half length 7 mm, the tip's sphere 7 mm further out) become spheres of the
    cylinder's radius at its centre -- a STATED DEVIATION of the kernel, not of the model: the description and the oracle keep the cylinder (MuJoCo's general convex
    collider, restated as GJK + EPA in oracle/jo_engine.c::collide_convex), and tests/test_gpu_leap.py measures what the stand-in costs at trajectory level."""
    if not any(g["type"] == "cylinder" for g in desc["geoms"]) or desc.get("family", desc["task"]) != "leap_cube":
        return desc
    out = dict(desc)
    out["geoms"] = [dict(g, type="sphere", size=[g["size"][0]], substitute_for_cylinder=list(g["size"])) if g["type"] == "cylinder" else g for g in desc["geoms"]]
    return out


def bounding_box_half(g: dict) -> np.ndarray:
    """Half sizes of the box around a geom in the geom's own frame (the broad phase's second level): a sphere's cube, a cylinder's (r, r, L), a box itself."""
    if g["type"] == "sphere":
        return np.array([g["size"][0]] * 3)
    if g["type"] == "cylinder":
        return np.array([g["size"][0], g["size"][0], g["size"][1]])
    return np.array(g["size"][:3])


# ---- pair tables of the hand's broad phase (jh_engine_v5.hip, level 1) ---------------------------------------------------------------------------------------
# A hand body pair whose relative pose depends on one or two hinge joints gets a bit grid over those joints' angles: a set bit says that NO pose in the cell can
# give the pair a level-2 candidate, and the kernel drops the pair before its box test.  Layout of the section (header slot HI_PT holds its offset; 0: none):
# [count, then PT_MAX records of PT_I ints: pair index, lane of joint 1, lane of joint 2, origin 1, 1 / cell width 1, origin 2, 1 / cell width 2 (float bits),
# the 64-bit word (low, high)]; bit ix + 8 * iy.  A single-joint table is a row: joint 2 = joint 1 with 1 / cell width 0 (iy = 0).  Unused records are zero.
PT_MAX, PT_I, PT_CELLS = 4, 9, 8
PT_SUB = 16        # sub-samples per cell and joint (cell midpoints of a PT_SUB x PT_SUB subdivision)
PT_MARGIN = 0.2    # rad by which the grid reaches beyond each joint's range on both sides (the limits are soft: a joint runs past them under load)
# What the table's bounds are widened by on top of the displacement bound D below: the kernel evaluates the same tests in fp32 in world coordinates -- operands
# below 1 m, chains of a few dozen operations at 6e-8 relative error each, rotation matrices accumulated over four links (1e-6, times a lever below 0.2 m) -- which
# stays below 1e-6 m; and it finds the cell as (int)((q - origin) * inv) in fp32, which can put an angle up to a few 1e-7 rad beyond a cell's edge into that cell:
# times a lever below 0.2 m, below 1e-7 m.  1e-5 m covers both ten times over.
PT_SLACK = 1e-5
PT_SUB_COARSE = (2, 4, 8)  # the coarser samplings a cell goes through first (see hand_pair_tables)
PT_CACHE = 8       # hand geometries whose tables are kept
_pt_cache: collections.OrderedDict[bytes, list] = collections.OrderedDict()


def _rot_axis(al: np.ndarray, q: np.ndarray) -> np.ndarray:
    """Rotation by q (N,) about the unit axis `al`, the kernel's expression."""
    sn, cs = np.sin(q), np.cos(q)
    t, (x, y, z) = 1.0 - cs, al
    return np.stack([t * x * x + cs, t * x * y - sn * z, t * x * z + sn * y, t * x * y + sn * z, t * y * y + cs, t * y * z - sn * x,
                     t * x * z - sn * y, t * y * z + sn * x, t * z * z + cs], -1).reshape(-1, 3, 3)


def _obb_faces(ca, Ra, ha, cb, Rb, hb, infl):
    """obb_face_overlap of the kernel over N poses, every one of the six bounds widened by `infl`."""
    d = cb - ca
    C = np.abs(np.einsum("nki,nkj->nij", Ra, Rb))
    da, db = np.abs(np.einsum("nki,nk->ni", Ra, d)), np.abs(np.einsum("nki,nk->ni", Rb, d))
    return (da <= ha + C @ hb + infl).all(-1) & (db <= hb + np.einsum("nki,k->ni", C, ha) + infl).all(-1)


def hand_pair_tables(F: list, I: list) -> list[dict]:
    """The pair tables of a leap-family image under construction (F, I as `pack_engine_model` has them behind the body-pair tables): at most PT_MAX dicts
    (pair, j1, j2, o1, inv1, o2, inv2, word, score), ascending in the pair index.

    Eligible: a pair (A, B) of the image's list whose relative pose is a function of one or two hinge joints -- the links on the tree path between them, A's side
    and B's side of their last common ancestor (static geometry: the world, no links).  The grid spans each joint's range widened by PT_MARGIN in PT_CELLS cells.

    Conservative by construction.  A cell is sampled at the midpoints of a PT_SUB x PT_SUB subdivision, so every pose of the closed cell lies within half a sample
    spacing, s_j / 2, of a sample in each joint.  Turning joint j by an angle a is, up to a rigid motion of the whole pair (which none of the tests sees), a rotation
    of B's side about the joint's anchor with A's side held, or of A's side with B's held: a point of either body at distance r from the anchor moves by at most
    a * r against the other body.  With L_j the largest distance, over all samples, from joint j's anchor to a point of either body's test volumes (each geom's
    centre plus the half diagonal of its box, each body's bounding-box centre plus its half diagonal), and D the largest displacement between a pose and its
    nearest sample, the distances on the way are at most L_j + 2 D (anchor and point each move by at most D), so D <= sum_j s_j / 2 * (L_j + 2 D), that is
    D <= sum_j s_j / 2 * L_j / (1 - sum_j s_j).  Every test of levels 1 and 2 is a comparison |projection of a centre difference| <= bound or |distance| <= bound,
    in which a box enters through the interval its points project to: the rotation of the boxes themselves is the displacement of their corners, which L_j
    covers.  So a test that passes at a pose passes at its nearest sample with the bound widened by D, and the tests are evaluated at the samples with every
    bound widened by D + PT_SLACK.  A cell is safe when no sample in it then passes level 1 and yields a level-2 candidate.  The argument holds for any sampling
    with its own D, so a cell is first sampled at the coarser spacings of PT_SUB_COARSE (each with its larger D): what one of them proves safe is safe, and only the rest
    is sampled PT_SUB x PT_SUB.  A pair whose bounding volumes overlap nowhere on the grid is not evaluated further.

    The tables chosen are those with the most cells that are safe AND pass the unwidened level 1 at some sample -- the cells where the table saves the kernel work --
    ties to the lower pair index; pairs with no such cell get none."""
    Ff = np.asarray(F, np.float32).astype(np.float64)  # (the values the kernel reads)
    o = image_offsets(I)
    NM, NBLK, nv, nu, NG, oDofF, oGeomF, oGeomI = o.NM, o.NBLK, o.NV, o.NU, o.NG, o.oDofF, o.oGeomF, o.oGeomI
    oBP, oBS, nBP, oBG, NBC = o.oBP, o.oBS, o.NBP, o.oBG, BODY_CODES
    # The tables are a function of the pair list, the bodies' tree, frames, joint axes and ranges, the geoms' types, sizes and poses, and the bodies' bounding
    # volumes -- not of the cube, masses, gains or friction: images that differ in those alone (randomised physics) share one cache entry.  The cache is small and
    # bounded: an entry per hand geometry in use.
    bodies = Ff[HEADER_F: HEADER_F + NM * BODY_F].reshape(NM, BODY_F)[1:]
    geoms = Ff[oGeomF: oGeomF + NG * GEOM_F].reshape(NG, GEOM_F)
    key = b"".join(np.ascontiguousarray(x).tobytes() for x in (
        np.asarray(I[HEADER_I: HEADER_I + NM * BODY_I] + I[oGeomI: oGeomI + NG * GEOM_I] + I[oBP: oBG + 2 * NBC] + [NM, NBLK, nv, nu, NG], np.int64),
        bodies[:, BF_LPOS:BF_LPOS + 12], bodies[:, BF_AXIS:BF_AXIS + 3], Ff[oDofF + 6 * DOF_F: oDofF + nv * DOF_F].reshape(-1, DOF_F)[:, DF_LIMITED:DF_HI + 1],
        geoms[:, 0:GF_RBOUND + 1], Ff[oBS: oBS + BV_F * NBC]))
    if key in _pt_cache:
        _pt_cache.move_to_end(key)
        return _pt_cache[key]
    # (the half sizes below take a geom that is neither a sphere nor a cylinder for a box, as the kernel's builds do for the kinds the packer lets through)
    assert all(I[oGeomI + g * GEOM_I + 1] in (GBOX, GSPHERE, GCYLINDER) for g in range(NG)), "pair tables: a geom kind the broad phase's restatement does not know"
    static = lambda c: c == 0 or c >= NM  # noqa: E731
    par = lambda c: I[HEADER_I + c * BODY_I]  # noqa: E731

    def chain(c):  # the links from the static root down to link c
        out = []
        while not static(c) and c > 0:
            out.append(c)
            c = par(c)
        return out[::-1]

    def body_volumes(c):
        g0, n = I[oBG + 2 * c], I[oBG + 2 * c + 1]
        G = Ff[oGeomF + g0 * GEOM_F: oGeomF + (g0 + n) * GEOM_F].reshape(n, GEOM_F)
        ty = [I[oGeomI + (g0 + k) * GEOM_I + 1] for k in range(n)]
        half = np.array([[g[0]] * 3 if t == GSPHERE else ([g[0], g[0], g[1]] if t == GCYLINDER else list(g[0:3])) for g, t in zip(G, ty)])
        bb = Ff[oBS + BV_F * c: oBS + BV_F * (c + 1)]
        return dict(pos=G[:, 3:6], R=G[:, 6:15].reshape(n, 3, 3), half=half, rb=G[:, 15], ctr=bb[0:3], rad=bb[3], bhalf=bb[4:7])

    cand = []
    for pi in range(nBP):
        ca, cb = I[oBP + 2 * pi], I[oBP + 2 * pi + 1]
        la, lb = chain(ca), chain(cb)
        while la and lb and la[0] == lb[0]:
            la, lb = la[1:], lb[1:]
        links = la + lb
        if not 1 <= len(links) <= 2 or any(I[HEADER_I + k * BODY_I + 1] != JHINGE or Ff[oDofF + (5 + k) * DOF_F + DF_LIMITED] == 0 for k in links):
            continue
        # the grid
        lo = [Ff[oDofF + (5 + k) * DOF_F + DF_LO] - PT_MARGIN for k in links]
        w = [(Ff[oDofF + (5 + k) * DOF_F + DF_HI] + PT_MARGIN - l0) / PT_CELLS for k, l0 in zip(links, lo)]
        two = len(links) == 2
        ncell = PT_CELLS * (PT_CELLS if two else 1)
        A, B = body_volumes(ca), body_volumes(cb)

        def evaluate(cells, sub):
            """Per cell of `cells`, sampled sub x sub: some sample passes the widened level 1 and yields a widened level-2 candidate; some sample does with nothing
            widened; some sample passes the unwidened level 1; and the displacement bound D of this sampling."""
            k1, k2 = np.meshgrid(np.arange(sub), np.arange(sub if two else 1), indexing="ij")
            qs = {links[0]: (lo[0] + ((cells % PT_CELLS)[:, None] + (k1.ravel() + 0.5) / sub) * w[0]).ravel()}
            if two:
                qs[links[1]] = (lo[1] + ((cells // PT_CELLS)[:, None] + (k2.ravel() + 0.5) / sub) * w[1]).ravel()
            cell = np.repeat(np.arange(len(cells)), k1.size)
            N = cell.size

            def side(ls):  # pose of the side's body in the frame of the last common ancestor (the world if there is none), and its links' anchors
                R, P, anchors = np.broadcast_to(np.eye(3), (N, 3, 3)), np.zeros((N, 3)), []
                for k in ls:
                    bf = Ff[HEADER_F + k * BODY_F: HEADER_F + (k + 1) * BODY_F]
                    P = P + R @ bf[0:3]
                    anchors.append(P)
                    R = R @ bf[3:12].reshape(3, 3) @ _rot_axis(bf[BF_AXIS:BF_AXIS + 3], qs[k])
                return R, P, anchors

            (RA, pA, anA), (RB, pB, anB) = side(la), side(lb)
            cAw, cBw = pA + RA @ A["ctr"], pB + RB @ B["ctr"]
            gA, gB = pA[:, None] + np.einsum("nij,gj->ngi", RA, A["pos"]), pB[:, None] + np.einsum("nij,gj->ngi", RB, B["pos"])
            # the displacement bound D
            L = []
            for an in anA + anB:
                r = max(np.linalg.norm(cAw - an, axis=-1).max() + A["rad"], np.linalg.norm(cBw - an, axis=-1).max() + B["rad"])
                for g, V in ((gA, A), (gB, B)):
                    r = max(r, (np.linalg.norm(g - an[:, None], axis=-1) + np.linalg.norm(V["half"], axis=-1)).max())
                L.append(r)
            sp = [x / sub for x in w]
            D = sum(0.5 * s_ * r for s_, r in zip(sp, L)) / (1.0 - sum(sp))

            def level1(idx, infl):
                d = cAw[idx] - cBw[idx]
                idx = idx[(d * d).sum(-1) <= (A["rad"] + B["rad"] + infl) ** 2]
                return idx[_obb_faces(cAw[idx], RA[idx], A["bhalf"], cBw[idx], RB[idx], B["bhalf"], infl)]

            def candidate(idx, infl):  # the samples of `idx` that pass level 1 and yield a level-2 candidate, every bound widened by `infl`
                s1, out = level1(idx, infl), np.zeros(N, bool)
                if not s1.size:
                    return out

                def near(g, V, co, Ro, ho):  # a geom of one body against the other body's bounding box
                    e = np.maximum(np.abs(np.einsum("nki,ngk->ngi", Ro, g - co[:, None])) - ho, 0.0)
                    return (e * e).sum(-1) <= (V["rb"] + infl) ** 2
                nA, nB = near(gA[s1], A, cBw[s1], RB[s1], B["bhalf"]), near(gB[s1], B, cAw[s1], RA[s1], A["bhalf"])
                for a in range(nA.shape[1]):
                    for b in range(nB.shape[1]):
                        i = s1[nA[:, a] & nB[:, b] & ~out[s1]]
                        if not i.size:
                            continue
                        e = gA[i, a] - gB[i, b]
                        i = i[(e * e).sum(-1) <= (A["rb"][a] + B["rb"][b] + infl) ** 2]
                        if i.size:
                            out[i] = _obb_faces(gA[i, a], RA[i] @ A["R"][a], A["half"][a], gB[i, b], RB[i] @ B["R"][b], B["half"][b], infl)
                return out

            everything = np.arange(N)
            l1_plain = np.zeros(N, bool)
            l1_plain[level1(everything, 0.0)] = True
            unsafe = candidate(everything, D + PT_SLACK)
            certain = candidate(np.flatnonzero(unsafe), 0.0)  # (a candidate with nothing widened: no finer sampling will call the cell safe)
            n = len(cells)
            return np.bincount(cell, weights=unsafe, minlength=n) > 0, np.bincount(cell, weights=certain, minlength=n) > 0, np.bincount(cell, weights=l1_plain, minlength=n) > 0, D

        # coarse to fine: a cell that a coarser sampling (with its own, larger D) already proves safe is safe; only the others go on to the next, down to PT_SUB x PT_SUB
        cells = np.arange(ncell)
        unsafe, certain, useful, D = evaluate(cells, PT_SUB_COARSE[0])
        if not useful.any():
            continue  # (the bounding volumes never overlap on the grid: level 1 drops the pair by itself, a table would save nothing)
        for sub in PT_SUB_COARSE[1:] + (PT_SUB,):
            again = np.flatnonzero(unsafe & ~certain)  # (a cell with a candidate at a sample, nothing widened, stays unsafe: not sampled again)
            if again.size:
                u2, c2, f2, D = evaluate(again, sub)
                unsafe[again], certain[again], useful[again] = u2, c2, useful[again] | f2
        safe = ~unsafe
        word = sum(1 << int(c) for c in np.flatnonzero(safe))
        cand.append(dict(pair=pi, j1=links[0] - 1, j2=links[-1] - 1, o1=float(lo[0]), inv1=float(1.0 / w[0]), o2=float(lo[1]) if two else 0.0,
                         inv2=float(1.0 / w[1]) if two else 0.0, word=word, score=int((safe & useful).sum()), D=float(D)))
    best = sorted((t for t in cand if t["score"] > 0), key=lambda t: (-t["score"], t["pair"]))[:PT_MAX]
    out = sorted(best, key=lambda t: t["pair"])
    _pt_cache[key] = out
    while len(_pt_cache) > PT_CACHE:
        _pt_cache.popitem(last=False)
    return out


def pair_table_section(tables: list[dict]) -> list[int]:
    """The int section's table block (see HI_PT)."""
    bits = lambda x: int(np.float32(x).view(np.int32))  # noqa: E731
    s32 = lambda u: u - (1 << 32) if u >= 1 << 31 else u  # noqa: E731
    out = [len(tables)]
    for t in tables:
        out += [t["pair"], t["j1"], t["j2"], bits(t["o1"]), bits(t["inv1"]), bits(t["o2"]), bits(t["inv2"]), s32(t["word"] & 0xFFFFFFFF), s32(t["word"] >> 32)]
    return out + [0] * (PT_I * (PT_MAX - len(tables)))


def read_pair_tables(blob: bytes) -> list[dict]:
    """The pair tables of a packed image: dicts as `hand_pair_tables` returns them (without score), [] where the image has none."""
    Iv = blob_sections(blob)[1]
    o = int(Iv[HI_PT]) if Iv.size > HI_PT else 0
    out = []
    for t in range(int(Iv[o]) if o > 0 else 0):
        r = Iv[o + 1 + t * PT_I: o + 1 + (t + 1) * PT_I]
        f = r[3:7].view(np.float32)
        out.append(dict(pair=int(r[0]), j1=int(r[1]), j2=int(r[2]), o1=float(f[0]), inv1=float(f[1]), o2=float(f[2]), inv2=float(f[3]),
                        word=(int(r[7]) & 0xFFFFFFFF) | (int(r[8]) & 0xFFFFFFFF) << 32))
    return out


def pair_table_safe(t: dict, qa, qb) -> np.ndarray:
    """The kernel's lookup, in its fp32 arithmetic: does table `t` rule the pair out at joint angles (qa, qb)?  An angle off the grid, or a NaN, reads as unsafe."""
    f32 = np.float32
    with np.errstate(invalid="ignore"):
        fa = (np.asarray(qa, f32) - f32(t["o1"])) * f32(t["inv1"])
        fb = (np.asarray(qb, f32) - f32(t["o2"])) * f32(t["inv2"])
        inside = (fa >= 0) & (fa < PT_CELLS) & (fb >= 0) & (fb < PT_CELLS)
    bit = np.where(inside, fa, 0).astype(np.int64) + PT_CELLS * np.where(inside, fb, 0).astype(np.int64)
    word = np.array([(t["word"] >> k) & 1 for k in range(64)], bool)
    return inside & word[bit]


def pack_engine_model(desc: dict, fingertips: str | None = None, pair_tables: bool = True) -> bytes:
    """`pair_tables` (leap family): False packs the image without the hand's pair tables (`hand_pair_tables`); the kernel then tests every body pair.

    `fingertips` (leap family; default: the description's own "fingertips" entry, else "sphere"): "sphere" packs `kernel_stand_ins(desc)`, the image every
    build of the leap kernel runs; "cylinder" keeps the MJCF's cylinders -- type code 5, sizes (radius, half length), bounding radius sqrt(r^2 + L^2) -- for the
    cylinder build (jh_engine_v5_cyl.hip), which jh_model_create selects by itself when it finds one."""
    fingertips = desc.get("fingertips", "sphere") if fingertips is None else fingertips
    if fingertips not in ("sphere", "cylinder"):
        raise ValueError(f"fingertips must be 'sphere' or 'cylinder', got {fingertips!r}")
    keep_cyl = fingertips == "cylinder" and desc.get("family", desc["task"]) == "leap_cube"
    if not isinstance(desc.get("self_collision", False), bool):
        raise ValueError(f"self_collision must be a bool, got {desc['self_collision']!r}")
    if desc.get("self_collision", False) and desc.get("family", desc["task"]) != "fr3_pick":
        raise NotImplementedError("self_collision: only the fr3 kernel has a build selected by this entry (the leap kernel models the hand's own contacts by default)")
    if fingertips == "cylinder" and not keep_cyl:
        raise NotImplementedError("fingertips='cylinder': only the leap kernel has a cylinder build")
    for g in desc["geoms"]:
        if keep_cyl and g["type"] == "cylinder" and (len(g["size"]) != 2 or min(g["size"]) <= 0):
            raise NotImplementedError(f"geom {g.get('name')}: a cylinder's size is (radius, half length), both positive")
    kinds = ("box", "sphere", "cylinder") if keep_cyl else ("box", "sphere")  # what the leap kernel's narrow phase takes
    if not keep_cyl:
        desc = kernel_stand_ins(desc)
    orig = desc
    ref_frames = sensor_reference_frames(orig)
    dofw_o, bodyw_o = inverse_weights(orig)
    desc = fuse_fixed_bodies(orig)
    st = engine_structure(desc)
    lay, moving, midx, blocks = st["layout"], st["moving"], st["midx"], st["blocks"]
    o = desc["option"]
    dofw = dofw_o  # dof order is unchanged by fusing
    bodyw_geom = lambda g: bodyw_o[g.get("orig_body", g["body"])][0]  # noqa: E731  (contact diagApprox uses the geom's ORIGINAL body)
    _, bodyw = inverse_weights(desc)
    NM, NBLK = len(moving), len(blocks)
    if NM > MAX_MOVING or lay.nv > MAX_DOF or NBLK > MAX_BLOCKS or max(len(b) for b in blocks) > MAX_BLOCK_DOF:
        raise NotImplementedError("model exceeds the engine's compile-time limits")

    cube_geoms = [g for g in desc["geoms"] if g["body"] == st["free"]]
    if len(cube_geoms) != 1 or cube_geoms[0]["type"] != "box" or np.abs(cube_geoms[0]["pos"]).max() > 0:
        raise NotImplementedError("free body must carry exactly one box geom centred on the body origin")
    cube = cube_geoms[0]
    # contacts modelled: cube geom vs every other collision geom (hand self-collision: out of scope this round)
    others = [g for g in desc["geoms"] if g["body"] != st["free"] and g["type"] in kinds]
    # geoms sorted by owning body so that the kernel loads each body pose once
    others.sort(key=lambda g: (-1 if st["is_static"][g["body"]] else midx[g["body"]]))
    if len(others) > MAX_GEOM:
        raise NotImplementedError("too many collision geoms")

    I: list[int] = [0] * HEADER_I
    F: list[float] = [0.0] * HEADER_F
    integ = {"euler": 0, "implicitfast": 3}[o["integrator"]]
    cone = {"pyramidal": 0, "elliptic": 1}[o["cone"]]
    if integ != 3:
        raise NotImplementedError("engine kernels implement the implicitfast integrator (leap_cube / fr3_pick)")
    sites = desc["sites"]
    sens = desc["sensors"]
    for slot, val in ((HI_NM, NM), (HI_NBLK, NBLK), (HI_NV, lay.nv), (HI_NQ, lay.nq), (HI_NU, lay.nu), (HI_NG, len(others)), (HI_NSITE, len(sites)), (HI_NS, lay.ns), (HI_INTEG, integ),
                      (HI_CONE, cone), (HI_NSENS, len(sens))):
        I[slot] = val
    # contact solver parameters are shared by all geoms in these models (checked)
    uniform = all(g["solref"] == cube["solref"] and g["solimp"] == cube["solimp"] for g in others)
    for g in others:
        if g["condim"] != 3 or g["margin"] != 0 or g["gap"] != 0:
            raise NotImplementedError("engine assumes condim 3 and zero margin/gap")
    cK, cB = solref_to_kb(cube["solref"], cube["solimp"], o["timestep"])
    F[0:3] = [o["timestep"], o["impratio"], SOLVER_TOL]
    F[3:6] = o["gravity"]
    F[6:8] = [cK, cB]
    F[8:13] = clamp_solimp(cube["solimp"])
    fbody = desc["bodies"][st["free"]]
    F[13:17] = [fbody["mass"], *fbody["inertia"]]
    F[17:20] = cube["size"]
    F[20] = float(np.linalg.norm(cube["size"]))
    F[21] = bodyw_geom(cube)
    F[22] = float(SOLVER_MAX_ITER)
    F[23] = float(SOLVER_LS_TOL)

    # ---- moving bodies
    for i, b in enumerate(moving):
        body = desc["bodies"][b]
        j = lay.body_joints[b][0]
        jn = desc["joints"][j]
        jt = {"free": JFREE, "slide": JSLIDE, "hinge": JHINGE}[jn["type"]]
        p = body["parent"]
        if st["is_static"][p]:
            ppos, pquat = _static_world_pose(desc, p)
            lpos = ppos + quat_to_mat(pquat) @ np.array(body["pos"])
            lquat = quat_mul(pquat, body["quat"])
            par = -1
        else:
            lpos, lquat, par = np.array(body["pos"]), np.array(body["quat"]), midx[p]
        if jt != JFREE and np.abs(jn["pos"]).max() > 0:
            raise NotImplementedError("engine assumes joint anchors at the body origin")
        blk = st["block_of"].get(b, -1)
        I += [par, jt, lay.jnt_dofadr[j], lay.jnt_qposadr[j], blk, (b - blocks[blk][0]) if blk >= 0 else 0]
        lR = quat_to_mat(lquat / np.linalg.norm(lquat))
        iR = quat_to_mat(body["iquat"])
        F += [*lpos, *lR.reshape(-1), body["mass"], *body["ipos"], *iR.reshape(-1), *body["inertia"], *jn["axis"], bodyw[b][0]]
    assert len(F) == HEADER_F + NM * BODY_F and len(I) == HEADER_I + NM * BODY_I
    # ---- blocks
    for blk in blocks:
        d0 = lay.jnt_dofadr[lay.body_joints[blk[0]][0]]
        I += [midx[blk[0]], len(blk), d0, len(blk)]
    # ---- dofs
    act_kv = np.zeros(lay.nv)
    for a in desc["actuators"]:
        act_kv[lay.jnt_dofadr[a["joint"]]] += a["kv"] * a["gear"] ** 2
    for d in range(lay.nv):
        jn = desc["joints"][lay.dof_jnt[d]]
        fl = jn["frictionloss"]
        # friction-loss row: pos = 0 -> impedance = dmin, K = 0, B from solreffriction, R = (1-d)/d * invweight
        si = clamp_solimp(jn["solimpfriction"])
        imp0 = si[0] if not (si[0] == si[1] or si[2] <= MINVAL) else 0.5 * (si[0] + si[1])
        _, fB = solref_to_kb(jn["solreffriction"], jn["solimpfriction"], o["timestep"])
        fR = max(MINVAL, (1 - imp0) / imp0 * dofw[d])
        lK, lB = solref_to_kb(jn["solreflimit"], jn["solimplimit"], o["timestep"])
        rng = jn["range"] if (jn["range"] is not None and jn["type"] != "free") else None
        frc = jn["actuatorfrcrange"]
        F += [jn["damping"], jn["armature"], fl, fB, 1.0 / fR if fl > 0 else 0.0, dofw[d], float(rng is not None), *(rng or (0, 0)), lK, lB,
              *clamp_solimp(jn["solimplimit"]), float(frc is not None), *(frc or (0, 0)), act_kv[d]]
    assert len(F) == HEADER_F + NM * BODY_F + lay.nv * DOF_F
    # ---- actuators (position servos on joints)
    for a in desc["actuators"]:
        j = a["joint"]
        I += [lay.jnt_dofadr[j], lay.jnt_qposadr[j]]
        if a["forcerange"] is not None:
            raise NotImplementedError("actuator forcerange")
        F += [a["kp"] * a["gear"], a["kv"] * a["gear"], float(a["ctrlrange"] is not None), *(a["ctrlrange"] or (0, 0)), 0, 0, 0]
    # ---- collision geoms (vs the cube)
    mu_cube = cube["friction"][0]
    for g in others:
        b = g["body"]
        if st["is_static"][b]:
            bpos, bquat = _static_world_pose(desc, b)
            pos = bpos + quat_to_mat(bquat) @ np.array(g["pos"])
            R = quat_to_mat(quat_mul(bquat, g["quat"]))
            mb = -1
        else:
            pos, R, mb = np.array(g["pos"]), quat_to_mat(g["quat"]), midx[b]
        size = (list(g["size"]) + [0, 0, 0])[:3]
        rb = size[0] if g["type"] == "sphere" else float(np.linalg.norm(size))  # (cylinder: size = (r, L, 0), so this is sqrt(r^2 + L^2))
        mu = max(MINMU, max(g["friction"][0], mu_cube))
        I += [mb, GTYPE[g["type"]]]
        F += [*size, *pos, *R.reshape(-1), rb, mu, bodyw_geom(g), max(MINMU, g["friction"][0]), 0]
    # ---- sites + sensors
    for s in sites:
        b = s["body"]
        if st["is_static"][b]:  # world-fixed site: body index -1, world position
            bp, bq = _static_world_pose(desc, b)
            I += [-1]
            F += list(bp + quat_to_mat(bq) @ np.array(s["pos"]))
            continue
        I += [midx[b]]
        F += list(s["pos"])
    for s in sens:
        if s["type"] == "framepos" and s.get("reftype") is not None and s["objtype"] == "body":
            I += [6, midx[s["obj"]], s["adr"]]  # body position in the static reference frame (tail block I[HI_REF])
        elif s["type"] == "framequat":
            I += [7, midx[s["obj"]], s["adr"]]  # body orientation relative to the static reference quaternion
        elif s["type"] == "framepos" and s["objtype"] == "site":
            I += [0, s["obj"], s["adr"]]
        elif s["type"] == "framepos":
            I += [1, midx[s["obj"]], s["adr"]]
        elif s["type"] == "jointpos":
            I += [2, lay.jnt_qposadr[s["obj"]], s["adr"]]
        elif s["type"] == "framezaxis" and s.get("objtype") == "body":
            I += [3, midx[s["obj"]], s["adr"]]
        elif s["type"] == "framezaxis":
            I += [5, s["obj"], s["adr"]]  # z axis of a site frame (generic section carries the rotation)
        else:
            I += [4, 0, s["adr"]]  # geom distance: generic section
    # ---- cooperative kernel (16 lanes per rollout, one lane per finger link): per-lane list of geoms to broad-phase.
    # lane l tests the geoms of moving body 1+l; static geoms are dealt greedily to the least-loaded lanes.
    if NM - 1 == 16 and NBLK == 4 and uniform:  # leap_cube layout of the cooperative kernel (needs uniform contact parameters)
        lists: list[list[int]] = [[] for _ in range(16)]
        for gi, g in enumerate(others):
            b = g["body"]
            if not st["is_static"][b]:
                lists[midx[b] - 1].append(gi)
        for gi, g in enumerate(others):
            if st["is_static"][g["body"]]:
                min(lists, key=len).append(gi)
        lgm = max(len(x) for x in lists)
        I[HI_LANES], I[HI_LGM] = len(I), lgm
        for x in lists:
            I += x + [-1] * (lgm - len(x))
        # hand self-collision (jh_engine_v5.hip): candidate geom pairs between hand bodies after MuJoCo's static filters (same welded body, parent-child,
        # the 18 excludes), grouped by body pair; a bounding sphere per body (static geometry: one sphere in world coordinates)
        oidx = {id(g): i for i, g in enumerate(others)}
        og = [g for g in desc["geoms"] if g["type"] in kinds]
        hh = [(a, b) for a, b in generic_pairs(orig, dict(desc, geoms=og), st, cube_only=False) if st["free"] not in (og[a]["body"], og[b]["body"])]
        # hand "bodies" of the self-collision tables: 1..16 = finger links; the static geometry is one body (0) when all of it collides with the same links
        # (leap_cube: the palm), else one body per set of static geoms with the same partners (caltech_leap_cube: floor + hand mount, palm): 0, 17, 18, 19
        link_code = lambda g: midx[g["body"]]  # noqa: E731
        partners: dict[int, set] = {}
        for a, b in hh:
            for x, y in ((og[a], og[b]), (og[b], og[a])):
                if st["is_static"][x["body"]] and not st["is_static"][y["body"]]:
                    partners.setdefault(x["body"], set()).add(link_code(y))
        sgroups: list[frozenset] = []
        for g in others:
            if st["is_static"][g["body"]]:
                key = frozenset(partners.get(g["body"], ()))
                if key not in sgroups:
                    sgroups.append(key)
        if len(sgroups) > 4:
            raise NotImplementedError("more than four groups of static collision geometry")
        SCODES = [0, 17, 18, 19]
        NBC = BODY_CODES  # body codes in the image (jh_engine_v5.hip NBC)
        code = lambda g: SCODES[sgroups.index(frozenset(partners.get(g["body"], ())))] if st["is_static"][g["body"]] else link_code(g)  # noqa: E731
        is_static_code = lambda c: c == 0 or c > 16  # noqa: E731
        groups: dict[tuple[int, int], list[tuple[int, int]]] = {}
        for a, b in hh:
            ga, gb = og[a], og[b]
            if is_static_code(code(gb)) or (not is_static_code(code(ga)) and code(ga) > code(gb)):  # side A: static geometry, else the lower link
                ga, gb = gb, ga
            if is_static_code(code(gb)):
                continue  # (static against static never collides)
            groups.setdefault((code(ga), code(gb)), []).append((oidx[id(ga)], oidx[id(gb)]))
        # MuJoCo's static filters act on bodies and every collision geom of the hand has the same contype / conaffinity: a surviving body pair collides
        # all of A's geoms with all of B's, and the geoms of a body are contiguous in `others` -> the image carries the body pairs and one
        # (first geom, count) range per body, no geom-pair table
        rng = {}
        for c in range(NBC):
            idxs = [i for i, g in enumerate(others) if code(g) == c]
            assert not idxs or idxs == list(range(idxs[0], idxs[0] + len(idxs))), "geoms of a body must be contiguous"
            rng[c] = (idxs[0], len(idxs)) if idxs else (0, 0)
        for (ca, cb), lst in groups.items():
            assert len(lst) == rng[ca][1] * rng[cb][1] and rng[ca][1] + rng[cb][1] <= 16, (ca, cb, len(lst))
        I[HI_BP], I[HI_NBP] = len(I), len(groups)
        for (ca, cb) in groups:
            I += [ca, cb]
        for c in range(NBC):
            I += list(rng[c])
        I[HI_BS] = len(F)
        for c in range(NBC):  # per hand body (static geometry: in world coordinates): bounding sphere and bounding box of its collision geoms, body frame
            gs = [g for g in others if code(g) == c]
            if not gs:
                F += [0.0] * 8
                continue
            corners = []
            for g in gs:
                if is_static_code(c):
                    bpos, bquat = _static_world_pose(desc, g["body"])
                    gp, gR = bpos + quat_to_mat(bquat) @ np.array(g["pos"]), quat_to_mat(quat_mul(bquat, g["quat"]))
                else:
                    gp, gR = np.array(g["pos"]), quat_to_mat(g["quat"])
                hs = bounding_box_half(g)
                for sx in (-1, 1):
                    for sy in (-1, 1):
                        for sz in (-1, 1):
                            corners.append(gp + gR @ (hs * np.array([sx, sy, sz])))
            corners = np.array(corners)
            lo, hi = corners.min(0), corners.max(0)
            ctr, half = 0.5 * (lo + hi), 0.5 * (hi - lo)
            F += [*ctr, float(np.linalg.norm(half)), *half, 0.0]
        hand_tables = hand_pair_tables(F, I) if pair_tables else []
    else:
        hand_tables = []
    # ---- generic sections (reference kernel): every collision geom incl. the cube, explicit candidate pairs, joint
    # equalities, sensor frames with orientation, geom-distance sensors
    allg = [g for g in desc["geoms"] if g["type"] in kinds + ("capsule",)]
    gidx = {id(g): i for i, g in enumerate(allg)}
    pairs_all = generic_pairs(orig, dict(desc, geoms=allg), st)
    frames = []
    for sx in sites:
        if st["is_static"][sx["body"]]:  # world-fixed frame
            bp, bq = _static_world_pose(desc, sx["body"])
            frames.append(dict(body=-1, pos=list(bp + quat_to_mat(bq) @ np.array(sx["pos"])), quat=list(quat_mul(bq, sx.get("quat", [1, 0, 0, 0])))))
        else:
            frames.append(dict(body=midx[sx["body"]], pos=sx["pos"], quat=sx.get("quat", [1, 0, 0, 0])))
    dists = [sx for sx in sens if sx["type"] == "distance"]
    eqs = desc["equalities"]
    I[HI_GI], I[HI_GF] = len(I), len(F)
    I[HI_ABLATE], I[HI_ABLATE_N] = ABLATE
    I += [len(allg), len(pairs_all), len(eqs), len(frames), len(dists), len(sens), 0, 0]
    for g in allg:
        b = g["body"]
        if st["is_static"][b]:
            bpos, bquat = _static_world_pose(desc, b)
            pos = bpos + quat_to_mat(bquat) @ np.array(g["pos"])
            R = quat_to_mat(quat_mul(bquat, g["quat"]))
            mb = -1
        else:
            pos, R, mb = np.array(g["pos"]), quat_to_mat(g["quat"]), midx[b]
        size = (list(g["size"]) + [0, 0, 0])[:3]
        rb = size[0] if g["type"] == "sphere" else (size[0] + size[1] if g["type"] == "capsule" else float(np.linalg.norm(size)))
        I += [mb, GTYPE[g["type"]]]
        F += [*size, *pos, *R.reshape(-1), rb, max(MINMU, g["friction"][0]), bodyw_geom(g), 0, 0]
    for g in allg:  # per-geom solver parameters, mixed per contact (solref/solimp averaged, friction max)
        F += [*g["solref"], *clamp_solimp(g["solimp"]), 0.0]
    for a, b in pairs_all:
        I += [a, b]
    for e in eqs:
        j1, j2 = e["joint1"], e["joint2"]
        d1, d2 = lay.jnt_dofadr[j1], lay.jnt_dofadr[j2]
        if any(abs(x) > 0 for x in e["polycoef"][2:]):
            raise NotImplementedError("joint equality: only linear coupling")
        eK, eB = solref_to_kb(e["solref"], e["solimp"], o["timestep"])
        blk1 = st["block_of"][desc["joints"][j1]["body"]]
        if blk1 != st["block_of"][desc["joints"][j2]["body"]]:
            raise NotImplementedError("joint equality across blocks")
        d0 = lay.jnt_dofadr[lay.body_joints[blocks[blk1][0]][0]]
        I += [d1, d2, blk1, d1 - d0, d2 - d0]
        F += [e["polycoef"][0], e["polycoef"][1], eK, eB, *clamp_solimp(e["solimp"]), dofw[d1] + dofw[d2], 0, 0]
    for fr in frames:
        I += [fr["body"]]
        F += [*fr["pos"], *quat_to_mat(fr["quat"]).reshape(-1)]
    glists: list[int] = []
    for sx in dists:
        la = [gidx[id(g)] for g in allg if g["orig_body"] == sx["body1"] and g["type"] == "box"]
        lb = [gidx[id(g)] for g in allg if g["orig_body"] == sx["body2"] and g["type"] == "box"]
        I += [len(glists), len(la), len(glists) + len(la), len(lb)]
        glists += la + lb
        F += [sx["cutoff"]]
    idist = 0
    for sx in sens:  # generic sensor table: (type, object, aux, address)
        if sx["type"] == "framepos" and sx.get("reftype") is not None and sx["objtype"] == "body":
            I += [6, midx[sx["obj"]], 0, sx["adr"]]
        elif sx["type"] == "framequat":
            I += [7, midx[sx["obj"]], 0, sx["adr"]]
        elif sx["type"] == "framepos" and sx.get("objtype") == "site":
            I += [0, sx["obj"], 0, sx["adr"]]
        elif sx["type"] == "framepos":
            I += [1, midx[sx["obj"]], 0, sx["adr"]]
        elif sx["type"] == "jointpos":
            I += [2, lay.jnt_qposadr[sx["obj"]], 0, sx["adr"]]
        elif sx["type"] == "framezaxis" and sx.get("objtype") == "site":
            I += [5, sx["obj"], 0, sx["adr"]]
        elif sx["type"] == "framezaxis":
            I += [3, midx[sx["obj"]], 0, sx["adr"]]
        else:
            I += [4, idist, 0, sx["adr"]]
            idist += 1
    I += glists
    if ref_frames is not None:  # reference frames of the sensors (jh_engine_v5.hip, caltech_leap_cube layout)
        I[HI_REF] = len(F)
        F += ref_frames
    if hand_tables:  # behind everything else in the int section, found through header slot HI_PT (zero in an image without tables): no other offset moves
        I[HI_PT] = len(I)
        I += pair_table_section(hand_tables)
    ntp = 9 if desc.get("family", desc["task"]) == "leap_cube" else 22
    return _pack(TASK_KIND[desc.get("family", desc["task"])], lay, ntp, F, I)


def geom_order(desc: dict) -> list[str]:
    """Names of the collision geoms in the order the engine tests them (for diagnostics)."""
    st = engine_structure(desc)
    others = [g for g in desc["geoms"] if g["body"] != st["free"] and g["type"] in ("box", "sphere")]
    others.sort(key=lambda g: (-1 if st["is_static"][g["body"]] else st["midx"][g["body"]]))
    return [g["name"] for g in others]
