"""Test infrastructure: the device narrow-phase routines of `judo_amd/csrc/jh_coop.h`, one pair of free-standing shapes per lane.

`tests/libjudo_amd_xcheck.so` exports `jh_xcheck_collide_pairs` (judo_amd/csrc/jh_xcheck_pairs.hip; no header declares it, it is not product interface).  This module
binds it with ctypes, builds its input rows and holds what the routine-level tests share: the shapes (every number rounded to fp32 FIRST, the rotation matrix built in
fp64 from the rounded, renormalised quaternion -- the kernel gets fp32(R), the references the fp64 values of the same numbers), the random generator of
`tests/test_oracle_independent.py::test_narrow_phase_agrees_with_support_function_geometry`, and the references: `tests/independent.py` (support-function geometry that
shares nothing with either implementation) and the oracle's routine with a measure of its own stability.
"""

from __future__ import annotations

import ctypes as C
import zlib
from dataclasses import dataclass, field

import numpy as np

from tests import independent as I

TYPE = {"sphere": 2, "capsule": 3, "cylinder": 5, "box": 6}  # MuJoCo's geom types, as CvxShape.type has them
ROUTINE = {"box_box": 0, "box_sphere": 1, "box_capsule": 2, "cylinder_sphere": 3, "convex": 4, "capsule_capsule": 5, "box_box_distance": 6}
PAIR_F, ROWS, ROW_F = 32, 24, 7


def quat_to_R(q: np.ndarray) -> np.ndarray:
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)], [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def _f32(x) -> np.ndarray:
    return np.asarray(x, dtype=np.float64).astype(np.float32).astype(np.float64)


def axis_angle(axis, angle: float) -> np.ndarray:
    a = np.asarray(axis, dtype=np.float64); a = a / np.linalg.norm(a)
    return np.concatenate([[np.cos(0.5 * angle)], np.sin(0.5 * angle) * a])


@dataclass
class Geom:
    """A shape whose every number is an fp32 value held in fp64.  size: box half extents (3), sphere (r), capsule / cylinder (r, half length along local z)."""

    kind: str
    size: np.ndarray
    pos: np.ndarray
    quat: np.ndarray
    R: np.ndarray = field(init=False)

    def __post_init__(self) -> None:
        self.size, self.pos = _f32(np.atleast_1d(self.size)), _f32(self.pos)
        q = _f32(self.quat)
        self.quat = q / np.linalg.norm(q)
        self.R = quat_to_R(self.quat)

    def moved(self, dpos, rotvec) -> "Geom":
        """The same shape displaced in fp64 (no rounding: the oracle's stability is probed around the exact inputs)."""
        g = Geom(self.kind, self.size, self.pos, self.quat)
        a = np.linalg.norm(rotvec)
        dq = axis_angle(rotvec, a) if a > 0 else np.array([1.0, 0, 0, 0])
        w1, v1, w2, v2 = dq[0], dq[1:], self.quat[0], self.quat[1:]
        g.quat = np.concatenate([[w1 * w2 - v1 @ v2], w1 * v2 + w2 * v1 + np.cross(v1, v2)])
        g.R, g.pos = quat_to_R(g.quat), self.pos + np.asarray(dpos)
        return g

    def shape(self) -> I.Shape:
        return I.Shape(self.kind, self.size, self.pos, self.R)

    def row(self) -> np.ndarray:
        s = np.zeros(3); s[: len(self.size)] = self.size
        return np.concatenate([[TYPE[self.kind]], s, self.pos, self.R.reshape(9)])

    def largest(self) -> float:
        return float(max(np.abs(self.pos).max(), self.size.max()))


def scale_of(a: Geom, b: Geom) -> float:
    """Every absolute tolerance is stated for coordinates up to 0.1 m and grows linearly with the largest input number of the case beyond that (fp32 rounding is relative)."""
    return max(1.0, max(a.largest(), b.largest()) / 0.1)


# ------------------------------------------------------------------------------------------------ the kernel
_fn = None


def _entry():
    global _fn
    if _fn is None:
        from tests import xcheck

        f = xcheck.load().jh_xcheck_collide_pairs
        f.restype = C.c_int
        f.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        _fn = f
    return _fn


def launch(routine: str, pairs: list[tuple[Geom, Geom]]):
    """One launch: (contacts (n, 24, 7) as rows (pos, normal, dist), raw push counts (n))."""
    import torch

    from judo_amd import _lib

    n = len(pairs)
    rows = np.stack([np.concatenate([a.row(), b.row()]) for a, b in pairs]).astype(np.float32)
    assert rows.shape == (n, PAIR_F)
    d_in = torch.from_numpy(rows).cuda()
    d_out = torch.full((n, ROWS, ROW_F), float("nan"), dtype=torch.float32, device="cuda")
    d_cnt = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    _lib.check(_entry()(ROUTINE[routine], d_in.data_ptr(), n, d_out.data_ptr(), d_cnt.data_ptr(), torch.cuda.current_stream().cuda_stream), "jh_xcheck_collide_pairs")
    torch.cuda.synchronize()
    return d_out.cpu().numpy().astype(np.float64), d_cnt.cpu().numpy()


def collide(routine: str, pairs: list[tuple[Geom, Geom]]) -> list[list[tuple[float, np.ndarray, np.ndarray]]]:
    """Contacts per pair as [(dist, pos, normal a->b)], the oracle's `collide_pair` format.  Nothing may have been dropped: the raw count fits the rows."""
    out, cnt = launch(routine, pairs)
    assert (cnt >= 0).all() and (cnt <= ROWS).all(), cnt
    res = [[(float(out[i, k, 6]), out[i, k, 0:3].copy(), out[i, k, 3:6].copy()) for k in range(cnt[i])] for i in range(len(pairs))]
    assert all(np.isfinite(d) and np.isfinite(p).all() and np.isfinite(nn).all() for r in res for d, p, nn in r), "a contact that is not finite"
    return res


def box_distance(pairs: list[tuple[Geom, Geom]]):
    out, cnt = launch("box_box_distance", pairs)
    return out[:, 0, 0], cnt.astype(bool)


# ------------------------------------------------------------------------------------------------ random pairs
TIRE = "tire"  # the second size class of the cylinder routines: the Spot tire against robot geoms of decimetre size


def random_pairs(ka: str, kb: str, n: int = 220, size_class: str = "") -> list[tuple[Geom, Geom]]:
    """The oracle test's generator (random rotations, box half extents 1-5 cm, sphere radii 1-4 cm, capsule / cylinder radii 0.8-2 cm and half lengths 1-5 cm, centre
    distance uniform in 0-9 cm), seeded by the pair's name (stable across processes).  `TIRE`: the cylinder is the spot_tire object, the other geom 3-12 cm thick and up to
    20 cm long, the centre distance uniform in 0-55 cm."""
    from judo_amd.spot_tasks import TIRE_HALF_WIDTH, TIRE_RADIUS

    rng = np.random.default_rng(zlib.crc32("-".join((ka, kb) + ((size_class,) if size_class else ())).encode()))
    tire = size_class == TIRE

    def mk(kind):
        q = rng.standard_normal(4); q /= np.linalg.norm(q)
        if kind == "box":
            size = rng.uniform(0.03, 0.12, 3) if tire else rng.uniform(0.01, 0.05, 3)
        elif kind == "sphere":
            size = np.array([rng.uniform(0.03, 0.12) if tire else rng.uniform(0.01, 0.04)])
        elif kind == "cylinder" and tire:
            size = np.array([TIRE_RADIUS, TIRE_HALF_WIDTH])
        else:
            size = np.array([rng.uniform(0.03, 0.08), rng.uniform(0.05, 0.2)]) if tire else np.array([rng.uniform(0.008, 0.02), rng.uniform(0.01, 0.05)])
        return kind, size, q

    out = []
    for _ in range(n):
        A, B = mk(ka), mk(kb)
        pb = rng.standard_normal(3); pb *= rng.uniform(0.0, 0.55 if tire else 0.09) / np.linalg.norm(pb)
        out.append((Geom(A[0], A[1], np.zeros(3), A[2]), Geom(B[0], B[1], pb, B[2])))
    return out


# ------------------------------------------------------------------------------------------------ references
def oracle_contacts(a: Geom, b: Geom):
    from oracle import oracle as O

    return O.collide_pair(a.kind, a.size, a.pos, a.quat, b.kind, b.size, b.pos, b.quat)


def match(got, ref):
    """Contacts matched as sets by nearest position (greedy over the sorted distances; equal counts): [(got index, ref index)]."""
    if not got:
        return []
    D = np.array([[np.linalg.norm(g[1] - r[1]) for r in ref] for g in got])
    pairs, used_g, used_r = [], set(), set()
    for flat in np.argsort(D, axis=None):
        i, j = divmod(int(flat), len(ref))
        if i not in used_g and j not in used_r:
            pairs.append((i, j)); used_g.add(i); used_r.add(j)
    return pairs


@dataclass
class Reference:
    """What the tests compare a pair's contacts with; computed once per pair (about 35 ms, nearly all of it the sampled signed distance) and never changed."""

    sd: float                 # signed distance from support functions, hinted with the oracle's normals (a hint can only sharpen a maximum over directions)
    scale: float
    oracle: list              # the oracle's contacts of the same numbers in fp64
    stable: bool              # the oracle keeps its contact count, its contacts within 1e-4 m and its normals within 1e-3 under six displacements of 1e-6 m / 1e-6 rad
    normal_only: bool         # ... and only the normals' condition, which the issue's definition of stable does not have, leaves the trial out (the tests report how many)
    pos_spread: float         # how far the oracle's matched positions moved under those displacements at the most (its own feature ambiguity)


def reference(a: Geom, b: Geom, seed: int) -> Reference:
    ref = oracle_contacts(a, b)
    sd, _ = I.signed_distance(a.shape(), b.shape(), n_dirs=500, seed=seed, extra_dirs=[o[2] for o in ref] if ref else None)
    rng = np.random.default_rng(seed + 7919)
    stable, turned, spread = True, False, 0.0
    for _ in range(6):
        dp, dr = rng.standard_normal(3), rng.standard_normal(3)
        alt = oracle_contacts(a, b.moved(1e-6 * dp / np.linalg.norm(dp), 1e-6 * dr / np.linalg.norm(dr)))
        if len(alt) != len(ref):
            stable = False
            break
        for i, j in match(alt, ref):
            dpos = float(np.linalg.norm(alt[i][1] - ref[j][1]))
            spread = max(spread, dpos)
            # (a normal that turns by more than 1e-3 under 1e-6 m turns by more than 1e-5 under the 1e-8 m of fp32 input rounding: the comparison to 1e-5 would test the conditioning)
            if dpos > 1e-4 or abs(alt[i][0] - ref[j][0]) > 1e-4:
                stable = False
            if np.abs(alt[i][2] - ref[j][2]).max() > 1e-3:
                turned = True
    return Reference(sd=float(sd), scale=scale_of(a, b), oracle=ref, stable=stable and not turned, normal_only=stable and turned, pos_spread=spread)


def sharpen(sd: float, a: Geom, b: Geom, got) -> float:
    """The reference's signed distance with the kernel's own normals as further candidate directions (the oracle test does the same with the oracle's)."""
    for _, _, n in got:
        l = np.linalg.norm(n)
        if l > 0.5:
            sd = max(sd, I.separation_along(a.shape(), b.shape(), n / l))
    return sd


def box_distance_numpy(a: Geom, b: Geom) -> float:
    """Signed box-box distance as the largest separation over the 15 SAT axes, fp64."""
    dv, best = b.pos - a.pos, -np.inf
    axes = [a.R[:, i] for i in range(3)] + [b.R[:, j] for j in range(3)]
    for i in range(3):
        for j in range(3):
            L = np.cross(a.R[:, i], b.R[:, j])
            l2 = L @ L
            if l2 >= 1e-12:
                axes.append(L / np.sqrt(l2))
    for ax in axes:
        best = max(best, abs(dv @ ax) - np.abs(a.R.T @ ax) @ a.size - np.abs(b.R.T @ ax) @ b.size)
    return float(best)
