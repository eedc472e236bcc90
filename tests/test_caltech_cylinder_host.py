"""Host side of the cylinder build of the leap kernel (no GPU): the model image that keeps caltech_leap_cube's fingertip cylinders, and the default images, which must
not move by a byte."""

import struct
from collections import Counter

import numpy as np
import pytest

ENGINE_MODELS = ("leap_cube", "leap_cube_down", "caltech_leap_cube", "fr3_pick")
ALL_MODELS = ENGINE_MODELS + ("cartpole", "cylinder_push")


def _sections(blob: bytes):
    """(float section, int section) of a packed model (64-byte header: magic, version, kind, nq, nv, nu, ns, ntaskparam, nfloat, nint)."""
    nf, ni = struct.unpack_from("<2I", blob, 32)
    F = np.frombuffer(blob, dtype="<f4", count=nf, offset=64)
    I = np.frombuffer(blob, dtype="<i4", count=ni, offset=64 + 4 * nf)
    return F, I


def _geom_table(blob: bytes):
    """The leap kernel's geom records: (ints (NG, 2) = body, type; floats (NG, 20) = size 3, pos 3, R 9, bounding radius, ...)."""
    from judo_amd import engine_model as E

    F, I = _sections(blob)
    o = E.image_offsets(I)
    NG, oI, oF = o.NG, o.oGeomI, o.oGeomF
    return I[oI:oI + NG * E.GEOM_I].reshape(NG, E.GEOM_I), F[oF:oF + NG * E.GEOM_F].reshape(NG, E.GEOM_F)


def test_default_images_do_not_depend_on_the_new_argument():
    """Every model packs to the same bytes with the argument left out, with fingertips="sphere", and through `pack_model`; a description without cylinders packs to the
    same bytes with fingertips="cylinder" too (nothing to keep); `kernel_stand_ins` is what it was: the four cylinders as spheres of their radius."""
    from judo_amd.engine_model import kernel_stand_ins, pack_engine_model
    from judo_amd.models import load_description, pack_model

    for task in ALL_MODELS:
        desc = load_description(task)
        blob = pack_model(desc)
        if task in ENGINE_MODELS:
            assert pack_engine_model(desc) == blob and pack_engine_model(desc, fingertips="sphere") == blob, task
            assert pack_engine_model(kernel_stand_ins(desc)) == blob, task
    for task in ("leap_cube", "leap_cube_down"):
        desc = load_description(task)
        assert pack_engine_model(desc, fingertips="cylinder") == pack_model(desc), task
    desc = load_description("caltech_leap_cube")
    cyl = [g for g in desc["geoms"] if g["type"] == "cylinder"]
    assert len(cyl) == 4 and all(g["size"] == [0.014, 0.007] for g in cyl)
    si = kernel_stand_ins(desc)
    assert si is not desc and [g["name"] for g in si["geoms"]] == [g["name"] for g in desc["geoms"]]
    for g, s in zip(desc["geoms"], si["geoms"]):
        if g["type"] == "cylinder":
            assert s["type"] == "sphere" and s["size"] == [0.014] and s["substitute_for_cylinder"] == [0.014, 0.007] and s["pos"] == g["pos"] and s["quat"] == g["quat"]
        else:
            assert s is g
    assert kernel_stand_ins(load_description("leap_cube")) == load_description("leap_cube")
    types, _ = _geom_table(pack_model(desc))
    assert set(types[:, 1].tolist()) == {2, 6}  # the default image of caltech_leap_cube: boxes and spheres, no cylinder


def test_cylinder_image_keeps_the_four_fingertips_as_the_mjcf_has_them():
    from judo_amd import engine_model as E
    from judo_amd.models import load_description, pack_model

    desc = load_description("caltech_leap_cube")
    sph, cyl = pack_model(desc), E.pack_engine_model(desc, fingertips="cylinder")
    assert E.pack_engine_model(dict(desc, fingertips="cylinder")) == cyl and pack_model(dict(desc, fingertips="cylinder")) == cyl  # (how a task hands the choice to GpuModel)
    assert len(cyl) == len(sph) and cyl != sph
    ti_s, tf_s = _geom_table(sph)
    ti_c, tf_c = _geom_table(cyl)
    is_cyl = ti_c[:, 1] == E.GCYLINDER
    assert E.GCYLINDER == 5 and is_cyl.sum() == 4
    np.testing.assert_array_equal(ti_c[:, 0], ti_s[:, 0])  # the same geoms on the same bodies, in the same order
    np.testing.assert_array_equal(ti_c[~is_cyl], ti_s[~is_cyl])
    np.testing.assert_array_equal(tf_c[~is_cyl], tf_s[~is_cyl])
    assert (ti_s[is_cyl, 1] == E.GSPHERE).all()
    r, L = np.float32(0.014), np.float32(0.007)
    for rec, rec_s in zip(tf_c[is_cyl], tf_s[is_cyl]):
        assert rec[0] == r and rec[1] == L and rec[2] == 0.0
        assert abs(rec[15] - np.sqrt(0.014**2 + 0.007**2)) < 1e-9  # bounding radius
        np.testing.assert_array_equal(rec[3:15], rec_s[3:15])  # pose in the body frame
        np.testing.assert_array_equal(rec[16:], rec_s[16:])    # friction, inverse weight
        assert rec_s[0] == r and rec_s[15] == r
    np.testing.assert_array_equal(E.bounding_box_half(dict(type="cylinder", size=[0.014, 0.007])), [0.014, 0.014, 0.007])
    with pytest.raises(ValueError):
        E.pack_engine_model(desc, fingertips="capsule")
    with pytest.raises(NotImplementedError):
        E.pack_engine_model(load_description("fr3_pick"), fingertips="cylinder")
    bad = dict(desc, geoms=[dict(g, size=[0.014]) if g["type"] == "cylinder" else g for g in desc["geoms"]])
    with pytest.raises(NotImplementedError, match="radius, half length"):
        E.pack_engine_model(bad, fingertips="cylinder")


def test_cylinder_pairs_are_the_oracles():
    """`generic_pairs` on the description with its cylinders: the oracle's candidate pairs, 233 box-cylinder, 12 cylinder-sphere and 6 cylinder-cylinder of 1 955, the
    cube's pairs first.  The body-pair tables of the two images are the same: a cylinder meets what its stand-in met."""
    from judo_amd import engine_model as E
    from judo_amd.models import load_description
    from oracle import oracle as O

    desc = load_description("caltech_leap_cube")
    om = O.Model("caltech_leap_cube")
    okind = Counter(tuple(sorted((desc["geoms"][a]["type"], desc["geoms"][b]["type"]))) for a, b in om.pairs)
    assert len(om.pairs) == 1955 and okind[("box", "cylinder")] == 233 and okind[("cylinder", "sphere")] == 12 and okind[("cylinder", "cylinder")] == 6
    fused = E.fuse_fixed_bodies(desc)
    st = E.engine_structure(fused)
    og = [g for g in fused["geoms"] if g["type"] in ("box", "sphere", "cylinder")]
    pairs = E.generic_pairs(desc, dict(fused, geoms=og), st, cube_only=False)
    kind = Counter(tuple(sorted((og[a]["type"], og[b]["type"]))) for a, b in pairs)
    assert kind == okind
    names = lambda geoms, prs: {frozenset((geoms[a]["name"], geoms[b]["name"])) for a, b in prs}  # noqa: E731
    assert names(og, pairs) == names(desc["geoms"], om.pairs)
    # ranks: pairs with the cube, then pairs against static geometry, then pairs between two links -- the order in which a full pool drops them
    def rank(pr):
        ba, bb = og[pr[0]]["body"], og[pr[1]]["body"]
        return 0 if st["free"] in (ba, bb) else (1 if st["is_static"][ba] or st["is_static"][bb] else 2)
    ranks = [rank(p) for p in pairs]
    assert ranks == sorted(ranks) and ranks[0] == 0 and ranks[-1] == 2
    ncube = sum(r == 0 for r in ranks)
    assert sum("cylinder" in (og[a]["type"], og[b]["type"]) for a, b in pairs[:ncube]) == 4  # the cube against each fingertip
    # with the stand-ins the same pairs, sphere for cylinder
    si = E.kernel_stand_ins(desc)
    fs = E.fuse_fixed_bodies(si)
    ogs = [g for g in fs["geoms"] if g["type"] in ("box", "sphere")]
    assert E.generic_pairs(si, dict(fs, geoms=ogs), E.engine_structure(fs), cube_only=False) == pairs
    # the generic section (what the older kernel generations read) lists the cube's pairs alone: 4 of them box-cylinder
    cube_pairs = E.generic_pairs(desc, dict(fused, geoms=og), st)
    assert Counter(tuple(sorted((og[a]["type"], og[b]["type"]))) for a, b in cube_pairs)[("box", "cylinder")] == 4


def test_task_argument_selects_the_image():
    from judo_amd.engine_model import pack_engine_model
    from judo_amd.models import load_description, pack_model
    from judo_amd.tasks import CaltechLeapCube, get_registered_tasks

    desc = load_description("caltech_leap_cube")
    t = CaltechLeapCube()
    assert t.fingertips == "sphere" and "fingertips" not in t.desc and pack_model(t.desc) == pack_model(desc)
    c = CaltechLeapCube(fingertips="cylinder")
    assert c.fingertips == "cylinder" and pack_model(c.desc) == pack_engine_model(desc, fingertips="cylinder")
    assert c.name == t.name and type(c.config) is type(t.config) and np.array_equal(c.default_state(), t.default_state())
    assert get_registered_tasks()["caltech_leap_cube"][0]().fingertips == "sphere"  # what make_controller builds
    with pytest.raises(ValueError):
        CaltechLeapCube(fingertips="box")
