#!/usr/bin/env python3
"""Transcribe the four BASELINE task models into the build's own model-description JSON.

Runs ONLY in the build container: it reads the reference's MJCF files
(`/root/reference/judo/models/xml/{cartpole,cylinder_push,leap_cube,fr3_pick}.xml` and the
`leap_components/`, `fr3_components/` includes), resolves the MJCF
default classes / includes / `fromto` / `inheritrange` for the subset of MJCF these four files
use, and writes `judo_amd/models/<task>.json`.  The JSON holds numbers only (topology, frames,
inertias, joint/actuator/solver parameters, collision primitives, sensors) in this build's own
schema; it is data, the runtime never sees MJCF.  Semantics of every field follow the MuJoCo 3.5
XML reference (MuJoCo itself is absent from this image, see DESIGN.md "oracle").

Documented substitutions (collision meshes are not in the reference repo, `.MISSING_LARGE_BLOBS`):
  * leap fingertip meshes `tip` / `thumb_tip` -> spheres (see MESH_SUBSTITUTES below)
  * fr3 link collision meshes -> capsule/box fits (see MESH_SUBSTITUTES below)
"""

from __future__ import annotations

import json
import math
import os
import sys
import xml.etree.ElementTree as ET

REF_XML = "/root/reference/judo/models/xml"
OUT_DIR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "judo_amd", "models")

# MuJoCo documented defaults (XML reference, MuJoCo 3.5)
GEOM_DEFAULTS = dict(
    type="sphere", contype="1", conaffinity="1", condim="3", friction="1 0.005 0.0001", solref="0.02 1",
    solimp="0.9 0.95 0.001 0.5 2", margin="0", gap="0", density="1000", solmix="1", priority="0",
    pos="0 0 0", quat="1 0 0 0",
)
JOINT_DEFAULTS = dict(
    type="hinge", pos="0 0 0", axis="0 0 1", damping="0", armature="0", frictionloss="0", stiffness="0",
    ref="0", margin="0", solreflimit="0.02 1", solimplimit="0.9 0.95 0.001 0.5 2",
    solreffriction="0.02 1", solimpfriction="0.9 0.95 0.001 0.5 2",
)

# Collision-mesh substitutes: {mesh name: primitive (or list of primitives) in the geom's own frame}.  The fingertip meshes `tip` / `thumb_tip` are
# replaced by the primitives the reference itself uses for the same fingertip in its mesh-free hand model
# (judo/models/xml/caltech_leap_components/leap_rh.xml:131-132,175-176,219-220,259-260: a cylinder r = 14 mm, half length 7 mm, and a sphere r = 14 mm
# 7 mm further out); for the MESH the cylinder is taken as a second sphere of the same radius (sphere-swept segment: the two overlap into a capsule-like tip whose
# far end sits at the reference's `trace_*_tip` site, leap_hand.xml:120,252).
MESH_SUBSTITUTES = {
    "tip": [dict(type="sphere", size=[0.014], pos=[0.0, -0.027, 0.0145], quat=[1, 0, 0, 0]), dict(type="sphere", size=[0.014], pos=[0.0, -0.034, 0.0145], quat=[1, 0, 0, 0])],
    "thumb_tip": [dict(type="sphere", size=[0.014], pos=[0.0, -0.0375, -0.01425], quat=[1, 0, 0, 0]), dict(type="sphere", size=[0.014], pos=[0.0, -0.0445, -0.01425], quat=[1, 0, 0, 0])],
    # fr3 link hulls: capsules along the link axes (radius ~ hull half-width of the FR3 links), not used by
    # the shipped fr3_pick cost except through contacts; fingers' mesh hull -> box over the finger body.
    "link0_coll": dict(type="capsule", size=[0.07, 0.06], pos=[-0.04, 0, 0.06], quat=[0.7071068, 0, 0.7071068, 0]),
    # (link1: round 6 shortened it from half length 0.10 at z = -0.10: that hull reached 57 mm into link0's -- the one pair of non-excluded neighbours MuJoCo collides,
    # link0 being welded to the world -- which no real hull pair does at rest; now 8 mm clear of it at every joint angle, joint 1 turning about the capsule's own axis)
    "link1_coll": dict(type="capsule", size=[0.06, 0.065], pos=[0, 0, -0.07], quat=[1, 0, 0, 0]),
    "link2_coll": dict(type="capsule", size=[0.06, 0.06], pos=[0, -0.06, 0.0], quat=[0.7071068, 0.7071068, 0, 0]),
    "link3_coll": dict(type="capsule", size=[0.055, 0.07], pos=[0.03, 0, -0.07], quat=[1, 0, 0, 0]),
    "link4_coll": dict(type="capsule", size=[0.055, 0.05], pos=[-0.04, 0.04, 0.0], quat=[0.7071068, 0.7071068, 0, 0]),
    "link5_coll": dict(type="capsule", size=[0.05, 0.13], pos=[0, 0.03, -0.13], quat=[1, 0, 0, 0]),
    "link6_coll": dict(type="capsule", size=[0.045, 0.04], pos=[0.04, 0, 0.0], quat=[0.7071068, 0, 0.7071068, 0]),
    "link7_coll": dict(type="capsule", size=[0.04, 0.03], pos=[0, 0, 0.05], quat=[1, 0, 0, 0]),
    "hand_coll": dict(type="box", size=[0.032, 0.10, 0.034], pos=[0, 0, 0.032], quat=[1, 0, 0, 0]),
    "finger_0": dict(type="box", size=[0.0105, 0.0075, 0.027], pos=[0, 0.0115, 0.027], quat=[1, 0, 0, 0]),
}


def fl(s: str) -> list[float]:
    return [float(x) for x in s.split()]


def load_xml(path: str) -> ET.Element:
    """Parse an MJCF file, inlining <include file=.../> elements (relative to the including file)."""
    root = ET.parse(path).getroot()

    def expand(el: ET.Element, base: str, here: str) -> None:
        i = 0
        while i < len(el):
            ch = el[i]
            if ch.tag == "include":
                fn = os.path.join(base, ch.get("file"))
                if not os.path.exists(fn):  # (objects/tire/tire.xml names tire_defs.xml next to itself)
                    fn = os.path.join(here, ch.get("file"))
                inc = ET.parse(fn).getroot()
                expand(inc, base, os.path.dirname(fn))  # MuJoCo resolves nested includes relative to the top-level model file
                el.remove(ch)
                for k, sub in enumerate(list(inc)):
                    el.insert(i + k, sub)
                i += len(inc)
            else:
                expand(ch, base, here)
                i += 1

    expand(root, os.path.dirname(path), os.path.dirname(path))
    return root


class Defaults:
    """MJCF default classes: nested <default class=..> inherit from the enclosing class."""

    def __init__(self, root: ET.Element) -> None:
        self.cls: dict[str, dict[str, dict[str, str]]] = {"main": {}}
        for d in root.findall("default"):
            self._walk(d, "main", top=True)

    def _walk(self, d: ET.Element, parent: str, top: bool = False) -> None:
        name = d.get("class") or ("main" if top else None)
        if name is None:
            raise ValueError("nested default without class")
        if name not in self.cls or name == "main":
            base = {t: dict(a) for t, a in self.cls[parent].items()} if name != "main" else self.cls["main"]
            self.cls[name] = base
        for ch in d:
            if ch.tag == "default":
                continue
            self.cls[name].setdefault(ch.tag, {}).update(ch.attrib)
        for ch in d.findall("default"):
            self._walk(ch, name)

    def resolve(self, tag: str, el: ET.Element, childclass: str | None, builtin: dict[str, str] | None = None) -> dict[str, str]:
        cname = el.get("class") or childclass or "main"
        out = dict(builtin or {})
        out.update(self.cls.get(cname, {}).get(tag, {}))
        out.update({k: v for k, v in el.attrib.items() if k != "class"})
        return out


def quat_mul(a, b):
    return [
        a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3],
        a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2],
        a[0] * b[2] - a[1] * b[3] + a[2] * b[0] + a[3] * b[1],
        a[0] * b[3] + a[1] * b[2] - a[2] * b[1] + a[3] * b[0],
    ]


def quat_rot(q, v):
    w, x, y, z = q
    R = [
        [1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
        [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
        [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)],
    ]
    return [sum(R[i][j] * v[j] for j in range(3)) for i in range(3)]


def mat_to_quat(R):
    """Rotation matrix (rows) -> unit quaternion (w, x, y, z)."""
    t = R[0][0] + R[1][1] + R[2][2]
    if t > 0:
        s_ = math.sqrt(t + 1.0) * 2
        q = [0.25 * s_, (R[2][1] - R[1][2]) / s_, (R[0][2] - R[2][0]) / s_, (R[1][0] - R[0][1]) / s_]
    elif R[0][0] > R[1][1] and R[0][0] > R[2][2]:
        s_ = math.sqrt(1.0 + R[0][0] - R[1][1] - R[2][2]) * 2
        q = [(R[2][1] - R[1][2]) / s_, 0.25 * s_, (R[0][1] + R[1][0]) / s_, (R[0][2] + R[2][0]) / s_]
    elif R[1][1] > R[2][2]:
        s_ = math.sqrt(1.0 + R[1][1] - R[0][0] - R[2][2]) * 2
        q = [(R[0][2] - R[2][0]) / s_, (R[0][1] + R[1][0]) / s_, 0.25 * s_, (R[1][2] + R[2][1]) / s_]
    else:
        s_ = math.sqrt(1.0 + R[2][2] - R[0][0] - R[1][1]) * 2
        q = [(R[1][0] - R[0][1]) / s_, (R[0][2] + R[2][0]) / s_, (R[1][2] + R[2][1]) / s_, 0.25 * s_]
    return qnorm(q)


def qnorm(q):
    n = math.sqrt(sum(x * x for x in q))
    return [x / n for x in q]


def quat_z_to(vec):
    """Quaternion rotating +z onto `vec` (MuJoCo mju_quatZ2Vec), used for `fromto`."""
    n = math.sqrt(sum(x * x for x in vec))
    v = [x / n for x in vec]
    axis = [-v[1], v[0], 0.0]  # z x v
    s = math.sqrt(axis[0] ** 2 + axis[1] ** 2)
    if s < 1e-10:
        return [1, 0, 0, 0] if v[2] > 0 else [0, 1, 0, 0]
    ang = math.atan2(s, v[2])
    axis = [a / s for a in axis]
    return [math.cos(ang / 2)] + [a * math.sin(ang / 2) for a in axis]


def geom_inertia(g: dict) -> tuple[float, list[float]]:
    """mass, diagonal inertia (in the geom frame, about its centre) of a primitive; MuJoCo formulas."""
    t, s = g["type"], g["size"]
    if t == "plane":  # planes carry no mass
        return 0.0, [0.0, 0.0, 0.0]
    if t == "box":
        vol = 8 * s[0] * s[1] * s[2]
    elif t == "sphere":
        vol = 4 / 3 * math.pi * s[0] ** 3
    elif t == "cylinder":
        vol = math.pi * s[0] ** 2 * 2 * s[1]
    elif t == "capsule":
        vol = math.pi * s[0] ** 2 * 2 * s[1] + 4 / 3 * math.pi * s[0] ** 3
    else:
        raise ValueError(t)
    mass = g["mass"] if g.get("mass") is not None else g["density"] * vol
    if t == "box":
        I = [mass / 3 * (s[1] ** 2 + s[2] ** 2), mass / 3 * (s[0] ** 2 + s[2] ** 2), mass / 3 * (s[0] ** 2 + s[1] ** 2)]
    elif t == "sphere":
        I = [0.4 * mass * s[0] ** 2] * 3
    elif t == "cylinder":
        r, h = s[0], 2 * s[1]
        I = [mass * (3 * r * r + h * h) / 12] * 2 + [mass * r * r / 2]
    else:  # capsule: cylinder + two hemispherical caps
        r, h = s[0], 2 * s[1]
        m_cyl = mass * (math.pi * r * r * h) / vol
        m_sph = mass - m_cyl
        it = m_cyl * (3 * r * r + h * h) / 12 + m_sph * (0.4 * r * r + h * h / 4 + 3 * r * h / 8)
        ia = m_cyl * r * r / 2 + m_sph * 0.4 * r * r
        I = [it, it, ia]
    return mass, I


def _check_orientation_attributes(root: ET.Element) -> None:
    """The orientation attributes this compiler does not implement must not appear at all (rounds 1-3 silently dropped `euler` on nine geoms of the Spot arm):
    `axisangle` / `xyaxes` / `zaxis` anywhere, `euler` on anything but a geom."""
    for el in root.iter():
        for k in ("axisangle", "xyaxes", "zaxis"):
            if k in el.attrib:
                raise NotImplementedError(f"<{el.tag} name={el.get('name')!r}>: orientation attribute {k!r} is not implemented")
        if "euler" in el.attrib and el.tag != "geom":
            raise NotImplementedError(f"<{el.tag} name={el.get('name')!r}>: `euler` is implemented for geoms only")


def compile_model(xml_name: str, task: str, prepare=None) -> dict:
    root = load_xml(os.path.join(REF_XML, xml_name))
    if prepare is not None:  # a transcription's documented substitutions, applied to the inlined tree
        prepare(root)
    _check_orientation_attributes(root)
    dfl = Defaults(root)
    comp = {}
    for c in root.findall("compiler"):
        comp.update(c.attrib)
    if comp.get("angle", "degree") != "radian":
        # cartpole / cylinder_push declare no angle unit; they contain no angular attribute
        # (hinge ranges, euler) so the default unit (degree) is never applied.
        pass
    opt = {}
    flags = {}
    for o in root.findall("option"):
        opt.update(o.attrib)
        for f in o.findall("flag"):
            flags.update(f.attrib)
    # attributes whose only modelled value is MuJoCo's default: read here so that another value fails loudly instead of being dropped (tests/test_mjcf_audit.py)
    if opt.get("solver", "Newton") != "Newton":
        raise NotImplementedError(f"{xml_name}: <option solver={opt.get('solver')!r}>: the engines implement the Newton solver only")
    if comp.get("autolimits", "true") != "true":
        raise NotImplementedError(f"{xml_name}: <compiler autolimits={comp.get('autolimits')!r}>: limits are inferred from the presence of a range, as autolimits=true does")
    if float(opt.get("density", 0)) not in (0.0, 1.0) or "viscosity" in opt or "wind" in opt:
        # density="1" (spot_primitive/default.xml:6): the medium's drag (~0.1 N on a 32 kg robot at 1 m/s) is a STATED deviation; anything denser is not
        raise NotImplementedError(f"{xml_name}: <option density / viscosity / wind>: fluid forces are not modelled")
    for b in root.iter("body"):
        if float(b.get("gravcomp", 0)) != 0.0:
            raise NotImplementedError(f"{xml_name}: <body name={b.get('name')!r} gravcomp={b.get('gravcomp')!r}>: gravity compensation is not modelled")
    model: dict = {
        "task": task,
        "source": f"judo v0.0.7 judo/models/xml/{xml_name}",
        "option": {
            "timestep": float(opt.get("timestep", 0.002)),
            "integrator": opt.get("integrator", "Euler").lower(),
            "cone": opt.get("cone", "pyramidal"),
            "impratio": float(opt.get("impratio", 1.0)),
            "gravity": fl(opt.get("gravity", "0 0 -9.81")),
            "contact": flags.get("contact", "enable") == "enable",
        },
        "bodies": [dict(name="world", parent=-1, pos=[0, 0, 0], quat=[1, 0, 0, 0], mass=0.0, ipos=[0, 0, 0], iquat=[1, 0, 0, 0], inertia=[0, 0, 0], mocap=False)],
        "joints": [], "geoms": [], "sites": [], "actuators": [], "sensors": [], "excludes": [], "equalities": [],
    }
    body_id = {"world": 0}

    def walk(el: ET.Element, parent: int, childclass: str | None) -> None:
        for b in el.findall("body"):
            cc = b.get("childclass") or childclass
            bid = len(model["bodies"])
            name = b.get("name", f"body{bid}")
            body_id[name] = bid
            rec = dict(name=name, parent=parent, pos=fl(b.get("pos", "0 0 0")), quat=qnorm(fl(b.get("quat", "1 0 0 0"))), mocap=b.get("mocap", "false") == "true")
            model["bodies"].append(rec)
            geoms_here = []
            for ch in b:
                if ch.tag in ("joint", "freejoint"):
                    a = dfl.resolve("joint", ch, cc, JOINT_DEFAULTS) if ch.tag == "joint" else dict(JOINT_DEFAULTS, type="free", **ch.attrib)
                    jr = dict(
                        name=a.get("name", f"joint{len(model['joints'])}"), body=bid, type=a["type"], pos=fl(a["pos"]), axis=fl(a["axis"]),
                        damping=float(a["damping"]), armature=float(a["armature"]), frictionloss=float(a["frictionloss"]),
                        stiffness=float(a["stiffness"]), ref=float(a["ref"]), margin=float(a["margin"]),
                        range=None, actuatorfrcrange=None,
                        solreflimit=fl(a["solreflimit"]), solimplimit=fl(a["solimplimit"]),
                        solreffriction=fl(a["solreffriction"]), solimpfriction=fl(a["solimpfriction"]),
                    )
                    if jr["type"] != "free":
                        n = math.sqrt(sum(x * x for x in jr["axis"]))
                        jr["axis"] = [x / n for x in jr["axis"]]
                    # autolimits (MuJoCo >= 2.2.2 default): a `range` attribute implies limited unless limited="false"
                    if "range" in a and a.get("limited", "auto") != "false":
                        jr["range"] = fl(a["range"])
                    if "actuatorfrcrange" in a and a.get("actuatorfrclimited", "auto") != "false":
                        jr["actuatorfrcrange"] = fl(a["actuatorfrcrange"])
                    model["joints"].append(jr)
                elif ch.tag == "geom":
                    a = dfl.resolve("geom", ch, cc, GEOM_DEFAULTS)
                    g = dict(
                        name=a.get("name", f"geom{len(model['geoms'])}"), body=bid, type=a["type"], contype=int(a["contype"]), conaffinity=int(a["conaffinity"]),
                        condim=int(a["condim"]), friction=(fl(a["friction"]) + [0.005, 0.0001])[:3] if len(fl(a["friction"])) < 3 else fl(a["friction"]),
                        solref=fl(a["solref"]), solimp=fl(a["solimp"]), margin=float(a["margin"]), gap=float(a["gap"]), solmix=float(a["solmix"]),
                        priority=int(a["priority"]), density=float(a["density"]), mass=float(a["mass"]) if "mass" in a else None,
                        pos=fl(a["pos"]), quat=qnorm(fl(a["quat"])), mesh=a.get("mesh"),
                    )
                    fr = fl(a["friction"])
                    g["friction"] = [fr[0], fr[1] if len(fr) > 1 else 0.005, fr[2] if len(fr) > 2 else 0.0001]
                    if "euler" in a:
                        # `euler` (spot_primitive/arm.xml: nine collision geoms of the arm): the compiler's default sequence "xyz" = intrinsic rotations about x, the new y,
                        # the new z, i.e. q = qx (x) qy (x) qz; radians (the files that use it declare <compiler angle="radian">)
                        assert comp.get("angle", "degree") == "radian" and comp.get("eulerseq", "xyz") == "xyz", "euler: only radians and the default sequence are implemented"
                        ex, ey, ez = fl(a["euler"])
                        qx = [math.cos(ex / 2), math.sin(ex / 2), 0.0, 0.0]; qy = [math.cos(ey / 2), 0.0, math.sin(ey / 2), 0.0]; qz = [math.cos(ez / 2), 0.0, 0.0, math.sin(ez / 2)]
                        g["quat"] = qnorm(quat_mul(quat_mul(qx, qy), qz))
                    size = fl(a["size"]) if "size" in a else []
                    if "fromto" in a:
                        ft = fl(a["fromto"])
                        p0, p1 = ft[:3], ft[3:]
                        vec = [p1[i] - p0[i] for i in range(3)]
                        g["pos"] = [(p0[i] + p1[i]) / 2 for i in range(3)]
                        g["quat"] = quat_z_to(vec)
                        size = [size[0], math.sqrt(sum(x * x for x in vec)) / 2]
                    g["size"] = size
                    geoms_here.append(g)
                elif ch.tag == "site":
                    a = dfl.resolve("site", ch, cc, dict(pos="0 0 0", quat="1 0 0 0"))
                    model["sites"].append(dict(name=a["name"], body=bid, pos=fl(a["pos"]), quat=qnorm(fl(a["quat"]))))
            # inertial: explicit <inertial> wins; else sum of geoms with mass (single-geom bodies in these models)
            inert = b.find("inertial")
            if inert is not None:
                if inert.get("diaginertia") is not None:
                    rec.update(mass=float(inert.get("mass")), ipos=fl(inert.get("pos", "0 0 0")), iquat=qnorm(fl(inert.get("quat", "1 0 0 0"))), inertia=fl(inert.get("diaginertia")))
                else:  # fullinertia = Ixx Iyy Izz Ixy Ixz Iyz in the inertial frame: principal axes by eigen-decomposition (any right-handed principal frame is equivalent)
                    import numpy as _np
                    f = fl(inert.get("fullinertia"))
                    I = _np.array([[f[0], f[3], f[4]], [f[3], f[1], f[5]], [f[4], f[5], f[2]]])
                    w, V = _np.linalg.eigh(I)
                    if _np.linalg.det(V) < 0:
                        V[:, 2] = -V[:, 2]
                    q_local = mat_to_quat(V.tolist())
                    q0 = qnorm(fl(inert.get("quat", "1 0 0 0")))
                    rec.update(mass=float(inert.get("mass")), ipos=fl(inert.get("pos", "0 0 0")), iquat=qnorm(quat_mul(q0, q_local)), inertia=[float(x) for x in w])
            else:
                massive = []
                for g in geoms_here:
                    if g["type"] == "mesh":
                        continue
                    m, I = geom_inertia(g)
                    if m > 0:
                        massive.append((g, m, I))
                if len(massive) == 0:
                    rec.update(mass=0.0, ipos=[0, 0, 0], iquat=[1, 0, 0, 0], inertia=[0, 0, 0])
                elif len(massive) == 1:
                    g, m, I = massive[0]
                    rec.update(mass=m, ipos=list(g["pos"]), iquat=list(g["quat"]), inertia=I)
                else:  # several massive geoms: total mass, centre of mass, inertia about it (parallel axes), principal frame -- what MuJoCo's compiler does
                    import numpy as _np

                    def rotm(q):
                        return _np.array([quat_rot(q, e) for e in ([1, 0, 0], [0, 1, 0], [0, 0, 1])]).T

                    mt = sum(m for _, m, _ in massive)
                    com = sum(m * _np.array(g["pos"]) for g, m, _ in massive) / mt
                    It = _np.zeros((3, 3))
                    for g, m, I in massive:
                        R = rotm(g["quat"])
                        d = _np.array(g["pos"]) - com
                        It += R @ _np.diag(I) @ R.T + m * (d @ d * _np.eye(3) - _np.outer(d, d))
                    w, V = _np.linalg.eigh(It)
                    w, V = w[::-1], V[:, ::-1]  # MuJoCo orders the principal moments descending
                    if _np.linalg.det(V) < 0:
                        V[:, 2] = -V[:, 2]
                    rec.update(mass=float(mt), ipos=[float(x) for x in com], iquat=qnorm(mat_to_quat(V.tolist())), inertia=[float(x) for x in w])
            for g in geoms_here:
                if g["contype"] == 0 and g["conaffinity"] == 0:
                    continue  # visual-only
                if (g["contype"], g["conaffinity"]) != (1, 1):
                    # the runtime's pair lists (judo_amd/engine_model.py, judo_amd/tree_model.py::robot_pairs, oracle/oracle.py::collision_pairs) apply MuJoCo's body-level
                    # filters only: with every collision geom at contype = conaffinity = 1 the mask test (ct1 & ca2) || (ct2 & ca1) passes for every pair, which is the
                    # case in all shipped models; anything else would silently produce extra pairs
                    raise NotImplementedError(f"geom {g['name']}: contype / conaffinity {g['contype']} / {g['conaffinity']}: only 1 / 1 (collides) and 0 / 0 (visual) are modelled")
                parts = [g]
                if g["type"] == "mesh":
                    subs = MESH_SUBSTITUTES.get(g["mesh"])
                    if subs is None:
                        raise KeyError(f"collision mesh {g['mesh']} has no substitute")
                    subs = subs if isinstance(subs, list) else [subs]
                    parts = []
                    for i_sub, sub in enumerate(subs):  # substitutes are expressed in the mesh geom's frame
                        gg = dict(g)
                        gg["pos"] = [g["pos"][i] + quat_rot(g["quat"], sub["pos"])[i] for i in range(3)]
                        gg["quat"] = qnorm(quat_mul(g["quat"], sub["quat"]))
                        gg["type"], gg["size"] = sub["type"], list(sub["size"])
                        gg["substitute_for_mesh"] = g["mesh"]
                        if len(subs) > 1:
                            gg["name"] = f"{g['name']}_{i_sub + 1}"
                        parts.append(gg)
                # (caltech_leap_cube's fingertip cylinders, caltech_leap_components/leap_rh.xml:131,175,219,259, stay cylinders in the description: the oracle collides them
                # with its general convex routine as MuJoCo does; the leap KERNEL's stand-in for them is applied by its own packer, judo_amd/engine_model.py::kernel_stand_ins)
                for gg in parts:
                    for k in ("mesh", "density", "mass", "contype", "conaffinity"):
                        gg.pop(k, None)
                    model["geoms"].append(gg)
            walk(b, bid, cc)

    wb = root.find("worldbody")
    direct = [ch for ch in list(wb) if ch.tag in ("geom", "site")]
    if direct:  # geoms / sites attached to the world itself (e.g. a ground plane): carried by a jointless body at the origin
        fixtures = ET.SubElement(wb, "body", dict(name="world_fixtures", pos="0 0 0"))
        for ch in direct:
            wb.remove(ch)
            fixtures.append(ch)
    walk(wb, 0, None)

    joint_id = {j["name"]: i for i, j in enumerate(model["joints"])}
    for c in root.findall("contact"):
        for e in c.findall("exclude"):
            model["excludes"].append([body_id[e.get("body1")], body_id[e.get("body2")]])
    for eq in root.findall("equality"):
        for j in eq.findall("joint"):
            model["equalities"].append(dict(
                type="joint", joint1=joint_id[j.get("joint1")], joint2=joint_id[j.get("joint2")],
                polycoef=(fl(j.get("polycoef", "0 1 0 0 0")) + [0, 0, 0, 0, 0])[:5],
                solref=fl(j.get("solref", "0.02 1")), solimp=fl(j.get("solimp", "0.9 0.95 0.001 0.5 2")),
            ))
    for act in root.findall("actuator"):
        for p in act.findall("position"):
            a = dfl.resolve("position", p, None, dict(kp="1", kv="0", gear="1"))
            j = joint_id[a["joint"]]
            rec = dict(name=a.get("name"), joint=j, kp=float(a["kp"]), kv=float(a["kv"]), gear=fl(a["gear"])[0], ctrlrange=None, forcerange=None)
            if "ctrlrange" in a and a.get("ctrllimited", "auto") != "false":
                rec["ctrlrange"] = fl(a["ctrlrange"])
            if "inheritrange" in a and float(a["inheritrange"]) > 0:
                lo, hi = model["joints"][j]["range"]
                mid, rad = (lo + hi) / 2, (hi - lo) / 2 * float(a["inheritrange"])
                rec["ctrlrange"] = [mid - rad, mid + rad]
            if "forcerange" in a and a.get("forcelimited", "auto") != "false":
                rec["forcerange"] = fl(a["forcerange"])
            model["actuators"].append(rec)
    site_id = {s["name"]: i for i, s in enumerate(model["sites"])}
    adr = 0
    for sen in root.findall("sensor"):
        for s in sen:
            rec = dict(name=s.get("name"), type=s.tag, adr=adr)
            if s.tag in ("framepos", "framexaxis", "frameyaxis", "framezaxis"):
                rec.update(objtype=s.get("objtype"), obj=(site_id if s.get("objtype") == "site" else body_id)[s.get("objname")], dim=3)
                if s.get("refname") is not None:  # value expressed in the reference frame (framepos: R_ref' (p - p_ref))
                    rec.update(reftype=s.get("reftype"), ref=(site_id if s.get("reftype") == "site" else body_id)[s.get("refname")])
            elif s.tag == "framequat":  # orientation of the object frame relative to the reference frame: q_ref^-1 * q_obj
                rec.update(objtype=s.get("objtype"), obj=(site_id if s.get("objtype") == "site" else body_id)[s.get("objname")], dim=4)
                if s.get("refname") is not None:
                    rec.update(reftype=s.get("reftype"), ref=(site_id if s.get("reftype") == "site" else body_id)[s.get("refname")])
            elif s.tag == "jointpos":
                rec.update(obj=joint_id[s.get("joint")], dim=1)
            elif s.tag == "distance":
                rec.update(body1=body_id[s.get("body1")], body2=body_id[s.get("body2")], cutoff=float(s.get("cutoff", 0)), dim=1)
            else:
                raise NotImplementedError(s.tag)
            adr += rec["dim"]
            model["sensors"].append(rec)
    model["nsensordata"] = adr
    return model


def transcribe_spot_box() -> dict:
    """judo/models/xml/spot_box/robot.xml as a description: a CROSS-CHECK only.  The product derives `spot_box` from spot.json in code
    (judo_amd/models.py::spot_box_description) and no spot_box.json is written; tests/test_spot_box_host.py compares the two."""
    m = compile_model("spot_box/robot.xml", "spot_box")
    m["family"] = "spot"
    return m


def _tire_stand_in(root: ET.Element) -> None:
    """spot_tire/robot.xml as the product models it: tire.xml's second <worldbody> merged into the first (MuJoCo merges them), the 81 collision meshes
    (absent upstream) dropped, and the reference's primitive approximation `object_primitive_approx` made collidable with the meshes' class `tire_collision`."""
    wbs = root.findall("worldbody")
    for wb in wbs[1:]:
        for ch in list(wb):
            wbs[0].append(ch)
        root.remove(wb)
    for b in root.iter("body"):
        for g in list(b.findall("geom")):
            if g.get("class") == "tire_collision":
                b.remove(g)
            elif g.get("name") == "object_primitive_approx":
                g.set("class", "tire_collision")
                g.attrib.pop("rgba", None)


def transcribe_spot_tire() -> dict:
    """judo/models/xml/spot_tire/robot.xml with the cylinder stand-in for the tire's meshes (_tire_stand_in): a CROSS-CHECK of
    judo_amd/models.py::spot_tire_description, compared by tests/test_spot_tire_host.py; no spot_tire.json is written."""
    m = compile_model("spot_tire/robot.xml", "spot_tire", prepare=_tire_stand_in)
    m["family"] = "spot"
    return m


def main() -> None:
    os.makedirs(OUT_DIR, exist_ok=True)
    for xml_name, task in (("cartpole.xml", "cartpole"), ("cylinder_push.xml", "cylinder_push"), ("leap_cube.xml", "leap_cube"), ("fr3_pick.xml", "fr3_pick"),
                           ("leap_cube_palm_down.xml", "leap_cube_down"), ("caltech_leap_cube.xml", "caltech_leap_cube"), ("spot_primitive/robot.xml", "spot")):
        m = compile_model(xml_name, task)
        if task in ("leap_cube_down", "caltech_leap_cube"):
            m["family"] = "leap_cube"  # same hand topology (palm-down pose / the Caltech primitive hand): runs on the leap_cube kernels
        path = os.path.join(OUT_DIR, task + ".json")
        with open(path, "w") as f:
            json.dump(m, f, indent=None, separators=(",", ":"))
            f.write("\n")
        nq = sum(7 if j["type"] == "free" else 1 for j in m["joints"])
        nv = sum(6 if j["type"] == "free" else 1 for j in m["joints"])
        print(f"{task}: bodies={len(m['bodies'])} joints={len(m['joints'])} nq={nq} nv={nv} geoms={len(m['geoms'])} "
              f"act={len(m['actuators'])} ns={m['nsensordata']} -> {path}", file=sys.stderr)


if __name__ == "__main__":
    main()
