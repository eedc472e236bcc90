"""Host side of the self-collision build of the fr3 kernel (jh_engine_v6_self.hip): `FR3Pick(self_collision=True)` puts "self_collision" into its description,
`engine_model.generic_pairs` then lists every pair the MJCF leaves (fr3_components/fr3.xml:11-99: 190 after MuJoCo's static filters = `oracle.collision_pairs(desc)`)
with the default build's 78 as a prefix, and the default image stays what it was.  No GPU needed."""

import os
import re
import struct

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _pair_names(desc):
    """(geom name, geom name) per candidate pair of the image packed from `desc`, in image order, read back from the image itself."""
    from judo_amd.engine_model import fuse_fixed_bodies, pack_engine_model

    blob = pack_engine_model(desc)
    nf = struct.unpack_from("<I", blob, 32)[0]
    I = np.frombuffer(blob, dtype="<i4", offset=64 + 4 * nf)
    gi = int(I[13])
    nag, npair = int(I[gi]), int(I[gi + 1])
    allg = [g for g in fuse_fixed_bodies(desc)["geoms"] if g["type"] in ("box", "sphere", "capsule")]
    assert len(allg) == nag
    pr = I[gi + 8 + 2 * nag: gi + 8 + 2 * nag + 2 * npair].reshape(npair, 2)
    return [(allg[a]["name"], allg[b]["name"]) for a, b in pr], [(allg[a]["type"], allg[b]["type"]) for a, b in pr]


def test_full_image_pairs_are_the_oracles_190():
    from judo_amd.tasks import FR3Pick
    from oracle import oracle as O

    t = FR3Pick(self_collision=True)
    names, types = _pair_names(t.desc)
    om = O.Model("fr3_pick")  # default scope: every pair the MJCF leaves
    gn = [g["name"] for g in om.desc["geoms"]]
    assert om.pairs == O.collision_pairs(t.desc) and len(om.pairs) == 190
    assert len(names) == len(set(names)) == 190
    assert {tuple(sorted(p)) for p in names} == {tuple(sorted((gn[a], gn[b]))) for a, b in om.pairs}
    # geom order within a pair: a capsule second, and two capsules in the oracle's (= the model's) order -- the contact frame's tangents follow the normal's direction
    assert all(ta == "box" or (ta, tb) == ("capsule", "capsule") for ta, tb in types)
    oracle_order = {(gn[a], gn[b]) for a, b in om.pairs}
    assert all(p in oracle_order for p, tt in zip(names, types) if tt == ("capsule", "capsule"))
    assert sum(tt == ("capsule", "capsule") for tt in types) == 22


def test_default_image_pairs_are_scope_kernel_and_a_prefix_of_the_full_list():
    from judo_amd.tasks import FR3Pick
    from oracle import oracle as O

    dn, _ = _pair_names(FR3Pick().desc)
    fn, ft = _pair_names(FR3Pick(self_collision=True).desc)
    om = O.Model("fr3_pick", scope="kernel")
    gn = [g["name"] for g in om.desc["geoms"]]
    assert len(dn) == 78 and {tuple(sorted(p)) for p in dn} == {tuple(sorted((gn[a], gn[b]))) for a, b in om.pairs}
    assert fn[:78] == dn
    new = list(zip(fn[78:], ft[78:]))
    assert len(new) == 112 and sum(tt == ("capsule", "capsule") for _, tt in new) == 22 and sum(tt == ("box", "capsule") for _, tt in new) == 90


def test_default_image_is_unchanged_by_the_new_argument():
    from judo_amd.engine_model import pack_engine_model
    from judo_amd.models import load_description, pack_model
    from judo_amd.tasks import FR3Pick

    t = FR3Pick()
    assert t.self_collision is False and "self_collision" not in t.desc
    ref = pack_engine_model(load_description("fr3_pick"))
    assert pack_engine_model(t.desc) == ref == pack_model(t.desc)
    assert pack_engine_model(dict(t.desc, self_collision=False)) == ref
    full = pack_engine_model(FR3Pick(self_collision=True).desc)
    assert full != ref and len(full) == len(ref) + 4 * 2 * 112  # 112 more pair records and nothing else


def test_task_carries_the_entry_and_refuses_a_bad_value():
    from judo_amd.engine_model import pack_engine_model
    from judo_amd.models import load_description
    from judo_amd.tasks import FR3Pick

    t = FR3Pick(self_collision=True)
    assert t.self_collision is True and t.desc["self_collision"] is True
    assert "self_collision" not in load_description("fr3_pick")  # the shared description is not touched
    for bad in (1, 0, "yes", None, np.bool_(True)):
        with pytest.raises(ValueError, match="self_collision"):
            FR3Pick(self_collision=bad)
    with pytest.raises(ValueError, match="self_collision"):
        pack_engine_model(dict(load_description("fr3_pick"), self_collision="all"))
    with pytest.raises(NotImplementedError, match="self_collision"):
        pack_engine_model(dict(load_description("leap_cube"), self_collision=True))


def test_make_controller_builds_the_default_task(monkeypatch):
    """`make_controller("fr3_pick", ...)` constructs `FR3Pick()` -- no argument, so the default pair set (the controller itself needs a GPU: the constructor is recorded)."""
    from judo_amd import controller as Cn
    from judo_amd.tasks import FR3Pick

    seen = {}
    monkeypatch.setattr(Cn, "make_controller_for", lambda task, opt, device=None, group=None: seen.setdefault("task", task))
    Cn.make_controller("fr3_pick", "cem")
    assert type(seen["task"]) is FR3Pick and seen["task"].self_collision is False and "self_collision" not in seen["task"].desc


def test_header_and_ctypes_table_agree_on_the_new_entry():
    from judo_amd import _lib

    header = open(os.path.join(ROOT, "include", "judo_amd.h")).read()
    m = re.search(r"int\s+jh_model_fr3_build\s*\(\s*const\s+jh_model\s*\*\s*m\s*,\s*int\s*\*\s*out[^)]*\)\s*;", header)
    assert m and "4 ints" in m.group(0)
    import ctypes as C

    res, args = _lib._SIGNATURES["jh_model_fr3_build"]
    assert res is C.c_int and args == [C.c_void_p, C.POINTER(C.c_int)] and "jh_model_fr3_build" in _lib.EXPORTED_SYMBOLS
    assert re.search(r"int\s+jh_model_build\s*\([^)]*4 ints[^)]*\)", header)  # the existing report keeps its four ints
    if os.path.exists(_lib.LIB_PATH):
        assert hasattr(C.CDLL(_lib.LIB_PATH), "jh_model_fr3_build")
