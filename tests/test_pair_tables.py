"""The pair tables of the leap kernel's hand broad phase (judo_amd/engine_model.py::hand_pair_tables, jh_engine_v5.hip level 1): a bit grid over two joint angles per
table pair, a set bit = "no pose in this cell gives the pair a level-2 candidate".  A bit that is set where the pair can touch would drop contacts silently, so the tables
are held to a numpy restatement of the kernel's level-1 and level-2 tests, written here from the kernel's source and independent of the packer's own evaluation: the
whole hand's kinematics in world coordinates, in float32 as the kernel computes, and in float64 with every bound loosened by 1e-6.  Host only; the GPU side is
tests/test_gpu_leap_pair_tables.py."""

import copy
import ctypes

import numpy as np
import pytest

from judo_amd import engine_model as em
from judo_amd import models

CASES = {"leap_cube": ("leap_cube", "sphere"), "leap_cube_down": ("leap_cube_down", "sphere"), "caltech_sphere": ("caltech_leap_cube", "sphere"),
         "caltech_cylinder": ("caltech_leap_cube", "cylinder")}
FINGERS = ("if", "mf", "rf")
POSES = 20000
BEYOND = 0.3  # rad by which the table joints are drawn beyond the grid on both sides


def description(name):
    task, tips = CASES[name]
    d = models.load_description(task)
    return dict(d, fingertips="cylinder") if tips == "cylinder" else d


def sections(blob):
    nf = int(np.frombuffer(blob[:64], np.uint32)[8])
    return np.frombuffer(blob[64: 64 + 4 * nf], np.float32).copy(), np.frombuffer(blob[64 + 4 * nf:], np.int32).copy()


class Hand:
    """What the kernel reads from an image, and its broad-phase tests for one body pair over N hand poses."""

    def __init__(self, blob, dtype):
        F, I = sections(blob)
        self.F, self.I, self.dt = F.astype(dtype), I, dtype
        o = em.image_offsets(I)
        self.oDof, self.oGeomF, self.oGeomI, self.oBP, self.oBS, self.nBP, self.oBG = o.oDofF, o.oGeomF, o.oGeomI, o.oBP, o.oBS, o.NBP, o.oBG
        self.ranges = np.array([[F[self.oDof + (6 + l) * em.DOF_F + em.DF_LO], F[self.oDof + (6 + l) * em.DOF_F + em.DF_HI]] for l in range(16)], np.float64)

    def kinematics(self, q):
        """World pose of the 16 links (body codes 1..16) at joint angles q (N, 16): the kernel's chain walk."""
        dt, N = self.dt, len(q)
        q = q.astype(dt)
        sn, cs = np.sin(q), np.cos(q)
        pos, rot = {}, {}
        for c in range(4):
            P, R = np.zeros((N, 3), dt), np.broadcast_to(np.eye(3, dtype=dt), (N, 3, 3))
            for j in range(4):
                l = 4 * c + j
                bf = self.F[em.HEADER_F + (1 + l) * em.BODY_F: em.HEADER_F + (2 + l) * em.BODY_F]
                P = P + R @ bf[0:3]
                R0 = R @ bf[3:12].reshape(3, 3)
                x, y, z = bf[28:31]
                s, k = sn[:, l], cs[:, l]
                t = 1 - k
                Rq = np.stack([t * x * x + k, t * x * y - s * z, t * x * z + s * y, t * x * y + s * z, t * y * y + k, t * y * z - s * x, t * x * z - s * y, t * y * z + s * x,
                               t * z * z + k], -1).reshape(N, 3, 3)
                R = R0 @ Rq
                pos[1 + l], rot[1 + l] = P, R
        return pos, rot

    def body(self, c, pos, rot, N):
        """Pose of body code c (static geometry: the identity, its records are in world coordinates) and its test volumes."""
        I, F, dt = self.I, self.F, self.dt
        static = c == 0 or c > 16
        p = np.zeros((N, 3), dt) if static else pos[c]
        R = np.broadcast_to(np.eye(3, dtype=dt), (N, 3, 3)) if static else rot[c]
        g0, n = int(I[self.oBG + 2 * c]), int(I[self.oBG + 2 * c + 1])
        G = F[self.oGeomF + g0 * em.GEOM_F: self.oGeomF + (g0 + n) * em.GEOM_F].reshape(n, em.GEOM_F)
        half = []
        for k in range(n):
            ty = int(I[self.oGeomI + (g0 + k) * em.GEOM_I + 1])
            half.append([G[k, 0]] * 3 if ty == em.GSPHERE else ([G[k, 0], G[k, 0], G[k, 1]] if ty == em.GCYLINDER else list(G[k, 0:3])))
        bb = F[self.oBS + 8 * c: self.oBS + 8 * c + 8]
        return dict(p=p, R=R, gpos=G[:, 3:6], gR=G[:, 6:15].reshape(n, 3, 3), half=np.array(half, dt), rb=G[:, 15], ctr=bb[0:3], rad=bb[3], bhalf=bb[4:7])

    @staticmethod
    def obb(ca, Ra, ha, cb, Rb, hb, loose):
        d = cb - ca
        C = np.abs(np.einsum("nki,nkj->nij", Ra, Rb))
        ok = np.ones(len(d), bool)
        for i in range(3):
            da = np.abs(np.einsum("nk,nk->n", d, Ra[:, :, i]))
            ok &= da <= ha[i] + hb[0] * C[:, i, 0] + hb[1] * C[:, i, 1] + hb[2] * C[:, i, 2] + loose
            db = np.abs(np.einsum("nk,nk->n", d, Rb[:, :, i]))
            ok &= db <= hb[i] + ha[0] * C[:, 0, i] + ha[1] * C[:, 1, i] + ha[2] * C[:, 2, i] + loose
        return ok

    def candidates(self, pair, q, loose=0.0):
        """(passes level 1, yields a level-2 candidate) of body pair `pair` at the poses q (N, 16)."""
        N = len(q)
        pos, rot = self.kinematics(q)
        A, B = (self.body(int(self.I[self.oBP + 2 * pair + k]), pos, rot, N) for k in (0, 1))
        cA, cB = A["p"] + A["R"] @ A["ctr"], B["p"] + B["R"] @ B["ctr"]
        d = cA - cB
        l1 = ((d * d).sum(-1) <= (A["rad"] + B["rad"] + loose) ** 2) & self.obb(cA, A["R"], A["bhalf"], cB, B["R"], B["bhalf"], loose)
        gA = A["p"][:, None] + np.einsum("nij,gj->ngi", A["R"], A["gpos"])
        gB = B["p"][:, None] + np.einsum("nij,gj->ngi", B["R"], B["gpos"])

        def near(g, X, co, O):  # (a): a geom's centre against the other body's bounding box
            e = np.maximum(np.abs(np.einsum("nki,ngk->ngi", O["R"], g - co[:, None])) - O["bhalf"], 0)
            return (e * e).sum(-1) <= (X["rb"] + loose) ** 2
        nA, nB = near(gA, A, cB, B), near(gB, B, cA, A)
        nA = nA & nB.any(1)[:, None]  # (the kernel looks at side A only when something of B is near)
        hit = np.zeros(N, bool)
        for a in range(nA.shape[1]):
            for b in range(nB.shape[1]):
                dd = gA[:, a] - gB[:, b]
                m = nA[:, a] & nB[:, b] & ((dd * dd).sum(-1) <= (A["rb"][a] + B["rb"][b] + loose) ** 2)
                if m.any():
                    idx = np.flatnonzero(m)
                    hit[idx] |= self.obb(gA[idx, a], A["R"][idx] @ A["gR"][a], A["half"][a], gB[idx, b], B["R"][idx] @ B["gR"][b], B["half"][b], loose)
        return l1, l1 & hit


@pytest.fixture(scope="module", params=list(CASES))
def image(request):
    d = description(request.param)
    blob = em.pack_engine_model(d)
    tables = em.read_pair_tables(blob)
    names = [b["name"] for b in em.fuse_fixed_bodies(d)["bodies"]]
    st = em.engine_structure(em.fuse_fixed_bodies(d))
    code_name = {i: names[b] for b, i in st["midx"].items()}
    return dict(name=request.param, desc=d, blob=blob, tables=tables, code_name=code_name)


def finger_tables(image):
    """finger -> the table of its (*_bs, *_md) pair."""
    _, I = sections(image["blob"])
    out = {}
    for t in image["tables"]:
        a, b = (image["code_name"].get(int(I[em.image_offsets(I).oBP + 2 * t["pair"] + k])) for k in (0, 1))
        for f in FINGERS:
            if (a, b) == (f + "_bs", f + "_md"):
                out[f] = t
    return out


def test_the_three_base_to_middle_pairs_have_tables(image):
    ft = finger_tables(image)
    assert sorted(ft) == sorted(FINGERS), (image["name"], image["tables"])
    assert 3 <= len(image["tables"]) <= em.PT_MAX and [t["pair"] for t in image["tables"]] == sorted({t["pair"] for t in image["tables"]})
    for f, t in ft.items():  # the pair's pose is a function of the finger's `rot` and `pip` joints: the lanes of *_px and *_md
        names = [image["code_name"][1 + t["j1"]], image["code_name"][1 + t["j2"]]]
        assert names == [f + "_px", f + "_md"], names
    assert em.read_pair_tables(em.pack_engine_model(image["desc"], pair_tables=False)) == []
    a, b = sections(image["blob"]), sections(em.pack_engine_model(image["desc"], pair_tables=False))
    o = int(a[1][em.HI_PT])
    assert o == len(b[1]) and (a[0] == b[0]).all() and b[1][em.HI_PT] == 0  # behind everything else; nothing moved
    keep = np.arange(o) != em.HI_PT
    assert (a[1][:o][keep] == b[1][keep]).all()


def test_no_candidate_where_a_table_says_safe(image):
    """20 000 random hand poses per table: the table joints uniform over the grid and 0.3 rad beyond it on both sides, the other joints uniform over their ranges."""
    h32, h64 = Hand(image["blob"], np.float32), Hand(image["blob"], np.float64)
    for ti, t in enumerate(image["tables"]):
        rng = np.random.default_rng(100 + ti)
        q = rng.uniform(h64.ranges[:, 0], h64.ranges[:, 1], (POSES, 16))
        q[:, t["j1"]] = rng.uniform(t["o1"] - BEYOND, t["o1"] + em.PT_CELLS / t["inv1"] + BEYOND, POSES)
        if t["j2"] != t["j1"]:
            q[:, t["j2"]] = rng.uniform(t["o2"] - BEYOND, t["o2"] + em.PT_CELLS / t["inv2"] + BEYOND, POSES)
        q = q.astype(np.float32)  # (the angles the kernel would hold)
        safe = em.pair_table_safe(t, q[:, t["j1"]], q[:, t["j2"]])
        l1_32, c32 = h32.candidates(t["pair"], q)
        l1_64, c64 = h64.candidates(t["pair"], q.astype(np.float64), loose=1e-6)
        print(f"{image['name']} pair {t['pair']}: safe {safe.mean():.3f}, level 1 passes {l1_64.mean():.3f}, candidates {c64.mean():.3f}, safe and candidate {int((safe & c64).sum())} / {int((safe & c32).sum())}")
        assert 0.2 < safe.mean() < 0.95 and c64.any()  # the draw reaches both kinds of cell
        assert not (safe & c32).any() and not (safe & c64).any()


def test_angles_off_the_grid_read_as_unsafe(image):
    for t in image["tables"]:
        full = dict(t, word=(1 << 64) - 1)  # (even a table of ones)
        w1, w2 = em.PT_CELLS / t["inv1"], (em.PT_CELLS / t["inv2"] if t["inv2"] else 1.0)
        mid1, mid2 = t["o1"] + 0.5 * w1, t["o2"] + 0.5 * w2
        assert em.pair_table_safe(full, mid1, mid2)
        for q1 in (t["o1"] - 1e-3, t["o1"] + w1 + 1e-3, -7.0, 7.0, np.nan, np.inf):
            assert not em.pair_table_safe(full, q1, mid2)
        if t["j2"] != t["j1"]:
            for q2 in (t["o2"] - 1e-3, t["o2"] + w2 + 1e-3, -7.0, 7.0, np.nan, -np.inf):
                assert not em.pair_table_safe(full, mid1, q2)


def test_the_default_pose_and_its_neighbours_are_safe(image):
    from judo_amd.tasks import get_registered_tasks

    q0 = np.asarray(get_registered_tasks()[CASES[image["name"]][0]][0]().default_state(), np.float64)[7:23]
    for f, t in finger_tables(image).items():
        for d1 in (-1, 0, 1):
            for d2 in (-1, 0, 1):
                assert em.pair_table_safe(t, q0[t["j1"]] + d1 / t["inv1"], q0[t["j2"]] + d2 / t["inv2"]), (image["name"], f, d1, d2)


def _create(blob):
    from judo_amd import _lib

    L = _lib.lib()
    buf = ctypes.create_string_buffer(blob, len(blob))
    h = ctypes.c_void_p()
    rc = L.jh_model_create(buf, len(blob), 0, ctypes.byref(h))
    msg = (L.jh_last_error() or b"").decode()
    if rc == 0:
        L.jh_model_destroy(h)
    return rc, msg


def test_a_malformed_table_section_is_refused():
    """jh_model_create checks the block before it touches the device: the kernel indexes lanes and pair bits with what the records hold."""
    blob = em.pack_engine_model(models.load_description("leap_cube"))
    F, I = sections(blob)
    o, nbp = int(I[em.HI_PT]), em.image_offsets(I).NBP
    nan = int(np.float32(np.nan).view(np.int32))
    bad = {"count": (o, em.PT_MAX + 1), "negative count": (o, -1), "pair": (o + 1, nbp), "negative pair": (o + 1, -1), "order": (o + 1 + em.PT_I, int(I[o + 1])),
           "lane": (o + 2, 16), "lane 2": (o + 3, -1), "origin": (o + 4, nan), "cell width": (o + 5, 0), "cell width 2": (o + 7, nan), "offset": (em.HI_PT, len(I) - 3),
           "offset in the header": (em.HI_PT, 5)}
    for what, (at, value) in bad.items():
        J = I.copy()
        J[at] = value
        rc, msg = _create(blob[:64] + F.tobytes() + J.tobytes())
        assert rc == -4 and "pair table" in msg, (what, rc, msg)
    if int(I[o]) < em.PT_MAX:  # a record beyond the count must be zero
        J = I.copy()
        J[o + 1 + em.PT_I * int(I[o]) + 2] = 3
        rc, msg = _create(blob[:64] + F.tobytes() + J.tobytes())
        assert rc == -4 and "pair table" in msg, (rc, msg)
    rc, msg = _create(blob)  # the image as packed passes the check (without a GPU the device upload fails, which is another error)
    assert rc != -4 and "pair table" not in msg, (rc, msg)


def test_a_model_set_keeps_the_tables_only_where_their_inputs_agree():
    """jh_pair_tables_shared, the rule jh_model_set_create applies to its members: a perturbed hand geom turns the tables off, a perturbed cube does not."""
    from judo_amd import _lib

    L = _lib.lib()
    shared = lambda a, b: L.jh_pair_tables_shared(ctypes.create_string_buffer(a, len(a)), len(a), ctypes.create_string_buffer(b, len(b)), len(b))  # noqa: E731
    d0 = models.load_description("leap_cube")
    b0 = em.pack_engine_model(d0)
    assert shared(b0, b0) == 1

    def variant(edit):
        d = copy.deepcopy(d0)
        edit(d)
        return em.pack_engine_model(d)

    body = {b["name"]: i for i, b in enumerate(d0["bodies"])}

    def geom_size(d):  # a hand geom 1 % larger
        g = next(g for g in d["geoms"] if g["body"] == body["mf_md"] and g["type"] == "box")
        g["size"] = [1.01 * x for x in g["size"]]

    def cube(d):  # the cube 5 % larger and heavier, more friction, a stiffer servo
        g = next(g for g in d["geoms"] if g["body"] == body["cube"])
        g["size"] = [1.05 * x for x in g["size"]]
        g["friction"] = [1.2 * g["friction"][0], *g["friction"][1:]]
        d["bodies"][body["cube"]]["mass"] *= 1.05
        d["bodies"][body["cube"]]["inertia"] = [1.05 * x for x in d["bodies"][body["cube"]]["inertia"]]
        d["bodies"][body["if_px"]]["mass"] *= 1.1
        d["actuators"][0]["kp"] *= 1.1

    def frame(d):  # a link mounted 1 mm further out
        d["bodies"][body["rf_md"]]["pos"] = [d["bodies"][body["rf_md"]]["pos"][0] + 1e-3, *d["bodies"][body["rf_md"]]["pos"][1:]]

    b_cube = variant(cube)
    assert b_cube != b0 and shared(b0, b_cube) == 1 and shared(b_cube, b0) == 1
    assert shared(b0, variant(geom_size)) == 0
    assert shared(b0, variant(frame)) == 0
    assert shared(b0, em.pack_engine_model(d0, pair_tables=False)) == 0
    plain = em.pack_engine_model(d0, pair_tables=False)
    assert shared(plain, plain) == 1  # (nothing to share, nothing to turn off)
    assert L.jh_pair_tables_shared(ctypes.create_string_buffer(b"xx", 2), 2, ctypes.create_string_buffer(b0, len(b0)), len(b0)) < 0
