"""Each device narrow-phase routine of `judo_amd/csrc/jh_coop.h` alone, one pair of free-standing shapes per lane (tests/pairs.py, judo_amd/csrc/jh_xcheck_pairs.hip).

The physics tests reach these routines only through whole steps, where a wrong contact is diluted by the solver and the branch a state reaches is neither controlled nor
counted.  Here every routine is called on 220 random pairs (the generator of the oracle's own check, plus the Spot tire's size class for the cylinder routines) and on
designed degenerate pairs.

PRIMARY criterion, every overlapping trial: exact geometry from `tests/independent.py` (support functions, shares nothing with the kernels or the oracle) -- no contact
where the signed distance sd > 1e-6, at least one where sd < -2e-4, the deepest contact never deeper than sd (2e-6 of fp32 rounding; box-box may prefer a face axis by
5 %), the exact routines within 5e-6 + 2e-3 |sd| of sd, every point inside both shapes grown by 0.5 |dist| + 2e-6, unit normals to 1e-5, and the shapes really overlap
by `dist` along the normal (2e-6 + 1e-3 |dist|).  SECONDARY criterion, where the oracle's own answer is stable under displacements of 1e-6 m / 1e-6 rad: the same
contact count, positions and depths to 2e-6 m, normals to 1e-5 (fp32 rounding of a few dozen operations on <= 0.15 m coordinates is about 5e-7 m; 2e-6 is the project's
figure for fp32 rotations of O(1) vectors).  `collide_convex_cylinder` (fp32 GJK + EPA, stop 1e-6 m) is held to twice its measured depth, position and normal
errors instead (CVX_MEASURED below says why 1e-5 is out of its reach) and, on every overlapping trial, to the two-sided form of the overlap along its normal, which is
what its stop guarantees.  All absolute tolerances grow linearly with the largest input number of the case beyond 0.1 m.

The measured figures are in profiles/narrow_phase_pairs.md; every case prints its own before it asserts.
"""

import functools
import json
from collections import Counter

import numpy as np
import pytest

from tests import independent as I
from tests import pairs as P
from tests.conftest import record_margin

pytestmark = pytest.mark.gpu

CONVEX = ("convex",)  # collide_convex_cylinder, the bounded fp32 GJK + EPA: ONE instantiation (the tree kernel's tire build and the leap cylinder build both stop at 1 000 nm)
CVX_TOL = 1e-6       # its stop in metres (jh_coop.h)
# (routine, first shape, second shape, size class)
CASES = [("box_box", "box", "box", ""), ("box_sphere", "box", "sphere", ""), ("box_capsule", "box", "capsule", ""), ("capsule_capsule", "capsule", "capsule", ""),
         ("cylinder_sphere", "cylinder", "sphere", ""), ("cylinder_sphere", "cylinder", "sphere", P.TIRE)]
for _r in CONVEX:
    CASES += [(_r, "capsule", "cylinder", ""), (_r, "box", "cylinder", ""), (_r, "cylinder", "cylinder", ""), (_r, "capsule", "cylinder", P.TIRE), (_r, "box", "cylinder", P.TIRE)]

# The bounded fp32 GJK + EPA against the oracle's fp64 GJK + EPA on stable trials: the largest error measured on an MI355X per pair kind and size class
# (profiles/narrow_phase_pairs.md), as (depth in m, position in m beyond the oracle's own feature ambiguity, normal), the first two per 0.1 m of the case's largest input
# number.  The test asserts TWICE these.  The depth is never allowed more than the primary criterion's 5e-6 + 2e-3 |sd|.  Normal and position cannot meet the closed-form
# routines' 1e-5 / 2e-6 m: a supporting plane within the stop of a curved face of radius r may be tilted by sqrt(2 CVX_TOL / r) -- 1.6e-2 at the smallest radius here,
# 8 mm -- and the witness points move by the radius times that (stated deviations).  What the stop does guarantee is asserted on every overlapping
# trial, stable or not: along the reported normal the shapes overlap by `dist` to within CVX_TOL + 2e-6, from both sides, which pins the normal to that cone.
CVX_MEASURED = {("capsule", "cylinder", ""): (9.13e-7, 2.86e-4, 6.97e-3), ("box", "cylinder", ""): (7.41e-7, 8.38e-4, 5.65e-3), ("cylinder", "cylinder", ""): (8.73e-7, 3.81e-4, 7.72e-3),
                ("capsule", "cylinder", P.TIRE): (1.23e-6, 3.20e-4, 9.10e-3), ("box", "cylinder", P.TIRE): (2.84e-7, 3.34e-4, 1.72e-3)}


@functools.lru_cache(maxsize=None)
def _references(ka, kb, size_class):
    """The pairs of a case and their references: computed once, shared by the tests that run the same pairs, never changed."""
    prs = P.random_pairs(ka, kb, 220, size_class)
    return prs, [P.reference(a, b, t) for t, (a, b) in enumerate(prs)]


def _axes_angle(a, b):
    c = abs(float(a.R[:, 2] @ b.R[:, 2]))
    return float(np.arctan2(np.linalg.norm(np.cross(a.R[:, 2], b.R[:, 2])), c))


def check_random(routine, ka, kb, size_class, prs, refs, got_all, need=100):
    """The criteria of the module docstring on the contacts `got_all` (one list per pair).  Prints the counts and the largest errors, then asserts."""
    name = f"{routine}[{ka}-{kb}{'-' + size_class if size_class else ''}]"
    hist, overlapping, grazing, unstable, apart = Counter(), 0, 0, 0, 0
    err = dict(pos=0.0, depth=0.0, normal=0.0, cvx_depth=0.0, exact=0.0, two_sided=0.0)
    bad, normal_only = [], 0
    for t, ((a, b), ref, got) in enumerate(zip(prs, refs, got_all)):
        s, SA, SB = ref.scale, a.shape(), b.shape()
        sd = P.sharpen(ref.sd, a, b, got)
        if sd > 1e-6 * s:
            apart += 1
            assert len(got) == 0, (name, t, "a contact between shapes that are apart", sd, got)
            continue
        if sd > -2e-4 * s:
            grazing += 1
            continue
        overlapping += 1
        assert len(got) >= 1, (name, t, "no contact between overlapping shapes", sd)
        hist[len(got)] += 1
        deepest = min(g[0] for g in got)
        slack = 0.05 * abs(sd) if routine == "box_box" else 0.0
        assert deepest >= sd - slack - 2e-6 * s, (name, t, "deeper than the shapes overlap", deepest, sd)
        exact = (routine in ("box_sphere", "cylinder_sphere") + CONVEX or (routine == "box_capsule" and sd > -0.98 * b.size[0])
                 or (routine == "capsule_capsule" and sd > -0.98 * (a.size[0] + b.size[0])))
        if exact:
            err["exact"] = max(err["exact"], (abs(deepest - sd) - 2e-3 * abs(sd)) / s)
            assert abs(deepest - sd) < 5e-6 * s + 2e-3 * abs(sd), (name, t, "deepest contact against the signed distance", deepest, sd)
        for dist, pos, nrm in got:
            assert abs(np.linalg.norm(nrm) - 1) <= 1e-5, (name, t, "normal not of unit length", nrm)
            tol = 0.5 * abs(dist) + 2e-6 * s
            assert SA.contains(pos, tol=tol) and SB.contains(pos, tol=tol), (name, t, "contact point outside a shape", dist, pos)
            sep = I.separation_along(SA, SB, nrm / np.linalg.norm(nrm))
            assert sep <= dist + 2e-6 * s + 1e-3 * abs(dist), (name, t, "the shapes do not overlap by dist along the normal", dist, sep)
            if routine in CONVEX:  # and by no more: EPA stops when the closest face is a supporting plane within CVX_TOL (2e-6: fp32 rounding, as everywhere)
                err["two_sided"] = max(err["two_sided"], (dist - sep) / s)
                if dist - sep > CVX_TOL + 2e-6 * s and (ka, kb, size_class) not in POLYTOPE_EXHAUSTED:
                    bad.append((t, "overlap along the normal beyond dist", dist - sep, CVX_TOL + 2e-6 * s))
        # ---- against the oracle, where its own answer is stable
        if routine == "capsule_capsule" and 0.0 < _axes_angle(a, b) < 1e-3:
            unstable += 1  # the kernel's fp32 parallel test takes the two-contact branch here, the fp64 oracle does not (the comment at the threshold): primary only
            continue
        if not ref.stable:
            unstable += 1
            normal_only += ref.normal_only
            continue
        if len(got) != len(ref.oracle):
            bad.append((t, "contact count", len(got), len(ref.oracle)))
            continue
        for i, j in P.match(got, ref.oracle):
            dpos, ddist = float(np.linalg.norm(got[i][1] - ref.oracle[j][1])), abs(got[i][0] - ref.oracle[j][0])
            dn = float(np.abs(got[i][2] - ref.oracle[j][2]).max())
            if routine in CONVEX:
                # the position only to the oracle's own feature ambiguity (the routine's comment); the depth to the measured figure
                dpos = max(0.0, dpos - ref.pos_spread)
                err["cvx_depth"] = max(err["cvx_depth"], ddist / s)
                m_depth, m_pos, m_normal = CVX_MEASURED[(ka, kb, size_class)]
                dtol, ptol, ntol = min(2 * m_depth * s, 5e-6 * s + 2e-3 * abs(sd)), 2 * m_pos * s, 2 * m_normal
            else:
                dtol, ptol, ntol = 2e-6 * s, 2e-6 * s, 1e-5
                err["depth"] = max(err["depth"], ddist / s)
            err["pos"], err["normal"] = max(err["pos"], dpos / s), max(err["normal"], dn)
            if dpos > ptol:
                bad.append((t, "position", dpos, ptol))
            if ddist > dtol:
                bad.append((t, "depth", ddist, dtol))
            if dn > ntol:
                bad.append((t, "normal", dn, ntol))
    line = dict(case=name, trials=len(prs), apart=apart, grazing=grazing, overlapping=overlapping, left_out_of_oracle=unstable, left_out_by_normal_alone=normal_only, histogram=dict(sorted(hist.items())),
                max_pos=err["pos"], max_depth=err["depth"], max_normal=err["normal"], max_cvx_depth=err["cvx_depth"], max_exact_excess=err["exact"], max_beyond_dist=err["two_sided"], failures=len(bad))
    print("narrow-phase " + json.dumps(line))
    record_margin("narrow_phase", **{k: (json.dumps(v) if isinstance(v, dict) else v) for k, v in line.items()})
    assert overlapping >= need, (name, "too few overlapping trials were checked", overlapping)
    assert unstable + grazing <= 0.05 * overlapping, (name, "too many trials left out", unstable, grazing, overlapping)
    if routine == "box_box":
        assert all(hist[k] > 0 for k in range(1, 7)), (name, "box-box must reach every contact count from 1 to 6", dict(hist))
    if routine == "box_capsule":
        assert all(hist[k] > 0 for k in range(1, 4)), (name, "box-capsule must reach every contact count from 1 to 3", dict(hist))
    assert not bad, (name, "against the oracle (trial, what, observed, bound)", bad[:12], len(bad))


@pytest.mark.parametrize("routine,ka,kb,size_class", CASES, ids=["-".join(x for x in c if x) for c in CASES])
def test_random_pairs(gpu, routine, ka, kb, size_class):
    prs, refs = _references(ka, kb, size_class)
    check_random(routine, ka, kb, size_class, prs, refs, P.collide(routine, prs))


# Capsule against cylinder: both shapes curved, the Minkowski difference's faces doubly curved, and on 2 of the 306 overlapping pairs the 36 expansions the polytope has
# room for (CVX_MAXV = 40) run out before the stop is reached: the routine keeps the closest face found so far, as its comment says, and along that face's normal the
# shapes overlap by MORE than the reported depth -- 2.53e-5 m against the allowed 3e-6 (small class), 1.15e-5 m against 7.6e-6 (tire class, trial 26).  Cause confirmed on
# a scratch build with CVX_MAXV = 120: the figures fall to 9.6e-7 and 3.0e-7 m (and the tire class's normal error from 9.1e-3 to 1.6e-3).  The fix is a larger polytope in
# the two shipped kernels that call the routine, which costs them private memory and time and needs their benchmarks: not done here.
POLYTOPE_EXHAUSTED = {("capsule", "cylinder", ""): "2.53e-5 m > 3e-6 m", ("capsule", "cylinder", P.TIRE): "1.15e-5 m > 7.6e-6 m"}


@pytest.mark.xfail(strict=True, reason="collide_convex_cylinder, capsule-cylinder: EPA's 36 expansions (CVX_MAXV = 40) run out on a doubly curved contact before the 1e-6 m stop; the face kept is "
                   "not a supporting plane within the stop (2.53e-5 / 1.15e-5 m).  With CVX_MAXV = 120 it is (9.6e-7 / 3.0e-7 m).  The fix changes two shipped kernels; DESIGN.md section 8.")
@pytest.mark.parametrize("ka,kb,size_class", list(POLYTOPE_EXHAUSTED), ids=["-".join(x for x in k if x) for k in POLYTOPE_EXHAUSTED])
def test_convex_overlap_along_the_normal_is_within_the_stop(gpu, ka, kb, size_class):
    """The one check `test_random_pairs[convex-capsule-cylinder*]` leaves out, alone: along the reported normal the shapes overlap by no more than `dist` + CVX_TOL + 2e-6."""
    prs, refs = _references(ka, kb, size_class)
    worst = 0.0
    for (a, b), ref, got in zip(prs, refs, P.collide("convex", prs)):
        for dist, _, nrm in got:
            worst = max(worst, (dist - I.separation_along(a.shape(), b.shape(), nrm / np.linalg.norm(nrm)) - CVX_TOL) / ref.scale)
    print(f"narrow-phase convex[{ka}-{kb}-{size_class}]: overlap along the normal beyond dist + stop, per scale: {worst:.3e} (bound 2e-6)")
    assert worst <= 2e-6


def test_capsule_capsule_parallel_classes(gpu):
    """Side by side, overlapping.  Exactly parallel axes: both criteria (the oracle takes its parallel branch too).  Axes 3e-4 rad apart: the kernel's fp32 test takes the parallel branch and the
    fp64 oracle does not -- the primary criterion only."""
    rng = np.random.default_rng(5)
    exact_prs, near_prs = [], []
    for k in range(24):
        q = rng.standard_normal(4)
        r1, r2, l1, l2 = rng.uniform(0.008, 0.02, 2).tolist() + rng.uniform(0.01, 0.05, 2).tolist()
        side = rng.standard_normal(3)
        a = P.Geom("capsule", [r1, l1], np.zeros(3), q)
        side -= (side @ a.R[:, 2]) * a.R[:, 2]
        pb = side / np.linalg.norm(side) * (r1 + r2) * rng.uniform(0.3, 0.95) + a.R[:, 2] * rng.uniform(-0.03, 0.03)
        exact_prs.append((a, P.Geom("capsule", [r2, l2], pb, q)))  # (the same numbers through the same rounding: exactly the same axis)
        tilt = P.Geom("capsule", [r2, l2], pb, q).moved(np.zeros(3), 3e-4 * side / np.linalg.norm(side))
        near_prs.append((a, P.Geom("capsule", [r2, l2], pb, tilt.quat)))
    for prs, both in ((exact_prs, True), (near_prs, False)):
        got_all = P.collide("capsule_capsule", prs)
        for t, ((a, b), got) in enumerate(zip(prs, got_all)):
            if not both:
                assert 0.0 < _axes_angle(a, b) < 1e-3
            ref = P.reference(a, b, t)
            sd, s = P.sharpen(ref.sd, a, b, got), ref.scale
            assert sd < -2e-4 and 1 <= len(got) <= 2, (t, sd, got)
            # (never deeper than the overlap; not necessarily as deep: the parallel branch, MuJoCo's, tests the four segment ends only)
            assert min(g[0] for g in got) >= sd - 2e-6 * s, (t, got, sd)
            for dist, pos, nrm in got:
                assert abs(np.linalg.norm(nrm) - 1) <= 1e-5
                assert a.shape().contains(pos, tol=0.5 * abs(dist) + 2e-6 * s) and b.shape().contains(pos, tol=0.5 * abs(dist) + 2e-6 * s), (t, dist, pos)
                assert I.separation_along(a.shape(), b.shape(), nrm / np.linalg.norm(nrm)) <= dist + 2e-6 * s + 1e-3 * abs(dist), (t, dist)
            if both:
                assert len(got) == len(ref.oracle) == 2, (t, got, ref.oracle)
                for i, j in P.match(got, ref.oracle):
                    assert np.linalg.norm(got[i][1] - ref.oracle[j][1]) <= 2e-6 * s and abs(got[i][0] - ref.oracle[j][0]) <= 2e-6 * s, (t, got[i], ref.oracle[j])
                    assert np.abs(got[i][2] - ref.oracle[j][2]).max() <= 1e-5, (t, got[i], ref.oracle[j])


def test_box_box_distance_and_touching(gpu):
    """`box_box_distance` against a 15-axis fp64 restatement to 2e-6; `box_box_touching` equals distance <= 0 wherever |distance| > 2e-6 and is never false for a pair
    the independent signed distance calls overlapping by more than 2e-6."""
    prs, refs = _references("box", "box", "")
    dist, touching = P.box_distance(prs)
    want = np.array([P.box_distance_numpy(a, b) for a, b in prs])
    print(f"narrow-phase box_box_distance: max |distance - fp64| = {np.abs(dist - want).max():.3e}, touching {int(touching.sum())} of {len(prs)}")
    assert np.abs(dist - want).max() <= 2e-6
    clear = np.abs(want) > 2e-6
    assert clear.sum() >= 200 and (want[clear] <= 0).sum() >= 100
    assert (touching[clear] == (want[clear] <= 0)).all()
    overlapping = np.array([r.sd < -2e-6 for r in refs])
    assert touching[overlapping].all()


# ------------------------------------------------------------------------------------------------ designed degenerate pairs: known answers from the geometry itself
OFFSETS = (np.zeros(3), np.array([0.3, -0.2, 0.5]))  # the second puts fp32 vertices a few ulps on either side of the boundaries
ID = np.array([1.0, 0, 0, 0])


def merged(points, tol=1e-6):
    out = []
    for p in points:
        if not any(np.linalg.norm(p - q) < tol for q in out):
            out.append(np.asarray(p))
    return out


def assert_same_points(got_pts, want_pts, tol, what):
    got_pts, want_pts = merged(got_pts), merged(want_pts)
    for w in want_pts:
        assert any(np.linalg.norm(w - g) <= tol for g in got_pts), (what, "an expected point is missing", w, got_pts)
    for g in got_pts:
        assert any(np.linalg.norm(w - g) <= tol for w in want_pts), (what, "a point outside the expected set", g, want_pts)


def clip_convex(subject, clip):
    """Sutherland-Hodgman in the plane, fp64: vertices of (subject polygon) n (convex clip polygon, counter-clockwise)."""
    out = [np.asarray(p, dtype=np.float64) for p in subject]
    for k in range(len(clip)):
        c0, c1 = np.asarray(clip[k]), np.asarray(clip[(k + 1) % len(clip)])
        e, inp, out = c1 - c0, out, []
        side = lambda p: e[0] * (p[1] - c0[1]) - e[1] * (p[0] - c0[0])
        for i in range(len(inp)):
            p, q = inp[i], inp[(i + 1) % len(inp)]
            sp, sq = side(p), side(q)
            if sp >= 0:
                out.append(p)
            if (sp > 0 and sq < 0) or (sp < 0 and sq > 0):
                out.append(p + (q - p) * sp / (sp - sq))
    return out


def _face_pair(axis, sign, h1, h2, pen, lateral, yaw):
    """Box 2's face against face `sign * axis` of box 1 (at the origin, axis-aligned), faces parallel, overlapping by `pen`; box 2 turned by `yaw` about the normal and
    shifted by `lateral` in the face's plane.  Returns the two boxes and the expected contact points: the overlap polygon at mid-overlap."""
    u, v = (axis + 1) % 3, (axis + 2) % 3
    e = np.eye(3)
    b1 = P.Geom("box", h1, np.zeros(3), ID)
    p2 = sign * (h1[axis] + h2[axis] - pen) * e[axis] + lateral[0] * e[u] + lateral[1] * e[v]
    b2 = P.Geom("box", h2, p2, P.axis_angle(e[axis], yaw))
    rect = [(-b1.size[u], -b1.size[v]), (b1.size[u], -b1.size[v]), (b1.size[u], b1.size[v]), (-b1.size[u], b1.size[v])]
    quad = []
    for su, sv in ((-1, -1), (1, -1), (1, 1), (-1, 1)):
        c = b2.pos + b2.R @ (su * b2.size[u] * e[u] + sv * b2.size[v] * e[v])
        quad.append((c[u], c[v]))
    want = []
    for pu, pv in clip_convex(quad, rect):
        w = np.zeros(3); w[u], w[v] = pu, pv
        w[axis] = sign * (b1.size[axis] - 0.5 * (b1.size[axis] + b2.size[axis] - sign * b2.pos[axis]))
        want.append(w)
    return b1, b2, want


def _shifted(g, off):
    return P.Geom(g.kind, g.size, g.pos + off, g.quat)


BOX_FACE_CASES = {
    "equal rectangles": dict(h1=[0.02, 0.012, 0.008], h2=[0.02, 0.012, 0.008], lateral=(0.0, 0.0), yaw=0.0),
    "vertices on edges": dict(h1=[0.02, 0.012, 0.008], h2=[0.02, 0.012, 0.008], lateral=(0.005, 0.0), yaw=0.0),
    "turned 45 degrees": dict(h1=[0.015, 0.015, 0.015], h2=[0.015, 0.015, 0.015], lateral=(0.0, 0.0), yaw=np.pi / 4),
    "face inside face": dict(h1=[0.02, 0.018, 0.016], h2=[0.006, 0.005, 0.004], lateral=(0.003, -0.002), yaw=0.3),
}


@pytest.mark.parametrize("case", list(BOX_FACE_CASES))
def test_box_box_parallel_faces(gpu, case):
    """Face to face (the gripper pad case): all six face pairings, both orders, at the origin and offset.  The contacts are exactly the corners of the overlap polygon at
    mid-overlap, depth = the overlap, normal = the face's."""
    c, pen = BOX_FACE_CASES[case], 0.001
    prs, wants = [], []
    for off in OFFSETS:
        for axis in range(3):
            for sign in (1.0, -1.0):
                b1, b2, want = _face_pair(axis, sign, c["h1"], c["h2"], pen, c["lateral"], c["yaw"])
                n = sign * np.eye(3)[axis]
                prs.append((_shifted(b1, off), _shifted(b2, off))); wants.append(([w + off for w in want], n))
                prs.append((_shifted(b2, off), _shifted(b1, off))); wants.append(([w + off for w in want], -n))
    expected_count = {"equal rectangles": 4, "vertices on edges": 4, "turned 45 degrees": 8, "face inside face": 4}[case]
    for t, ((a, b), (want, n), got) in enumerate(zip(prs, wants, P.collide("box_box", prs))):
        s = P.scale_of(a, b)
        assert len(merged(want)) == expected_count, (case, t, want)
        assert_same_points([g[1] for g in got], want, 2e-6 * s, (case, t))
        for dist, pos, nrm in got:
            assert abs(dist + pen) <= 2e-6 * s and np.abs(nrm - n).max() <= 1e-4, (case, t, dist, nrm, n)


def test_box_box_crossed_edges_and_coincident_centres(gpu):
    prs = []
    h1, h2, pen = [0.04, 0.01, 0.01], [0.01, 0.04, 0.01], 0.001
    for off in OFFSETS:
        a = P.Geom("box", h1, off, P.axis_angle([1, 0, 0], np.pi / 4))     # its top edge runs along x at height sqrt(2) * 0.01
        b = P.Geom("box", h2, off + [0, 0, np.sqrt(2) * 0.02 - pen], P.axis_angle([0, 1, 0], np.pi / 4))  # its bottom edge runs along y
        prs += [(a, b), (b, a)]
    got_all = P.collide("box_box", prs)
    for t, ((a, b), got) in enumerate(zip(prs, got_all)):
        s, off, up = P.scale_of(a, b), OFFSETS[t // 2], 1.0 if t % 2 == 0 else -1.0
        assert len(got) == 1, (t, got)
        dist, pos, nrm = got[0]
        assert abs(dist + pen) <= 2e-6 * s and np.abs(nrm - [0, 0, up]).max() <= 1e-4, (t, got)
        assert np.linalg.norm(pos - (off + [0, 0, np.sqrt(2) * 0.01 - 0.5 * pen])) <= 2e-6 * s, (t, pos)
    # exactly coincident centres: the smaller box's face in the larger one's, along the axis of least total extent, either sign
    prs = [(P.Geom("box", [0.03, 0.02, 0.01], off, ID), P.Geom("box", [0.01, 0.012, 0.004], off, ID)) for off in OFFSETS]
    for t, ((a, b), got) in enumerate(zip(prs, P.collide("box_box", prs))):
        s = P.scale_of(a, b)
        assert len(merged([g[1] for g in got])) == 4, (t, got)
        for dist, pos, nrm in got:
            assert abs(dist + 0.014) <= 2e-6 * s and np.abs(np.abs(nrm) - [0, 0, 1]).max() <= 1e-4, (t, dist, nrm)
            rel = pos - a.pos
            assert np.abs(np.abs(rel[:2]) - [0.01, 0.012]).max() <= 2e-6 * s and abs(abs(rel[2]) - 0.003) <= 2e-6 * s, (t, rel)


TILT = P.axis_angle([0.3, -0.5, 0.8], 0.7)


def _local_cases(kind_a, size_a, quat_a, cases):
    """Pairs of a first shape at OFFSETS and second shapes given in its frame; `cases`: (second shape as (kind, size, local position), expected (dist, local normal,
    local position) or None).  Returns the pairs and the expectations in world coordinates."""
    prs, wants = [], []
    for off in OFFSETS:
        for (kind, size, local), want in cases:
            a = P.Geom(kind_a, size_a, off, quat_a)
            prs.append((a, P.Geom(kind, size, a.pos + a.R @ np.asarray(local, dtype=np.float64), ID)))
            wants.append(None if want is None else (want[0], a.R @ np.asarray(want[1], dtype=np.float64), a.pos + a.R @ np.asarray(want[2], dtype=np.float64)))
    return prs, wants


def _check_single(prs, wants, got_all, what):
    for t, ((a, b), want, got) in enumerate(zip(prs, wants, got_all)):
        s = P.scale_of(a, b)
        if want is None:
            assert got == [], (what, t, got)
            continue
        assert len(got) == 1, (what, t, got)
        dist, pos, nrm = got[0]
        assert abs(dist - want[0]) <= 2e-6 * s and np.abs(nrm - want[1]).max() <= 1e-4 and np.linalg.norm(pos - want[2]) <= 2e-6 * s, (what, t, got[0], want)


def test_box_sphere_designed(gpu):
    h, r = np.array([0.03, 0.02, 0.01]), 0.01
    cases = []

    def outside(c):
        c = np.asarray(c); q = np.clip(c, -h, h); l = np.linalg.norm(c - q); n = (c - q) / l
        return (("sphere", [r], c), (l - r, n, q + 0.5 * (l - r) * n))

    cases += [outside([0.005, 0.003, h[2] + 0.006]), outside([h[0] + 0.003, h[1] + 0.004, 0.002]), outside([h[0] + 0.002, -h[1] - 0.003, h[2] + 0.006])]
    for k in range(3):  # inside, nearest each of the six faces
        for sg in (1.0, -1.0):
            c = np.array([0.001, -0.0015, 0.0005]); c[k] = sg * (h[k] - 0.002)
            n = np.zeros(3); n[k] = sg
            q = c.copy(); q[k] = sg * h[k]
            cases.append((("sphere", [r], c), (-0.002 - r, n, q + 0.5 * (-0.002 - r) * n)))
    prs, wants = _local_cases("box", h, TILT, cases)
    _check_single(prs, wants, P.collide("box_sphere", prs), "box-sphere")
    # the centre exactly at the box's centre (a finite normal along the thinnest axis, either sign) and exactly on a face (axis-aligned: the numbers are exact in fp32)
    prs = [(P.Geom("box", h, off, TILT), P.Geom("sphere", [r], off, ID)) for off in OFFSETS]
    for t, ((a, b), got) in enumerate(zip(prs, P.collide("box_sphere", prs))):
        assert len(got) == 1 and abs(got[0][0] + h[2] + r) <= 2e-6 * P.scale_of(a, b), (t, got)
        assert min(np.abs(got[0][2] - a.R[:, 2]).max(), np.abs(got[0][2] + a.R[:, 2]).max()) <= 1e-4, (t, got)
    a = P.Geom("box", h, np.zeros(3), ID)
    prs = [(a, P.Geom("sphere", [r], [0.004, 0.002, a.size[2]], ID))]
    _check_single(prs, [(-r, np.array([0, 0, 1.0]), np.array([0.004, 0.002, a.size[2] - 0.5 * r]))], P.collide("box_sphere", prs), "box-sphere, centre on a face")


def test_box_capsule_designed(gpu):
    h, r = np.array([0.03, 0.02, 0.01]), 0.005
    along_x, s2 = P.axis_angle([0, 1, 0], np.pi / 2), np.sqrt(0.5)
    for off in OFFSETS:
        box = P.Geom("box", h, off, ID)
        s = 1.0 if not off.any() else 5.0
        flat = P.Geom("capsule", [r, 0.01], off + [0.002, 0.001, h[2] + 0.003], along_x)           # parallel to the top face, inside its outline
        across = P.Geom("capsule", [r, 0.02], off + [h[0] + 0.003 * s2, 0.004, h[2] + 0.003 * s2], P.axis_angle([0, 1, 0], 3 * np.pi / 4))  # across the edge x = hx, z = hz
        through = P.Geom("capsule", [r, 0.03], off + [0.01, 0.005, 0.0], ID)                        # through the box, both ends outside
        one_end = P.Geom("capsule", [r, 0.02], off + [0.01, 0.005, h[2] + 0.02 + r - 0.002], ID)    # the lower end 2 mm into the top face
        got = P.collide("box_capsule", [(box, flat), (box, across), (box, through), (box, one_end)])
        # flat: the two ends, and no third -- or an interior point of the same depth on the axis
        ends = [off + [0.002 + sg * 0.01, 0.001, h[2] - 0.001] for sg in (1, -1)]
        for e in ends:
            assert any(np.linalg.norm(e - g[1]) <= 2e-6 * s for g in got[0]), (off, "an end is missing", e, got[0])
        assert 2 <= len(got[0]) <= 3
        for dist, pos, nrm in got[0]:
            assert abs(dist + 0.002) <= 2e-6 * s and np.abs(nrm - [0, 0, 1]).max() <= 1e-4, (off, got[0])
            rel = pos - off
            assert abs(rel[0] - 0.002) <= 0.01 + 2e-6 * s and abs(rel[1] - 0.001) <= 2e-6 * s and abs(rel[2] - (h[2] - 0.001)) <= 2e-6 * s, (off, rel)
        # across: the interior point alone, against the edge
        n = np.array([s2, 0, s2])
        _check_single([(box, across)], [(-0.002, n, off + [h[0], 0.004, h[2]] - 0.001 * n)], [got[1]], ("box-capsule across an edge", off))
        # through: one contact (the interior point, a centre inside the box); its point and depth hold the geometric criteria
        assert len(got[2]) == 1, (off, got[2])
        dist, pos, nrm = got[2][0]
        assert dist <= -through.size[0] + 2e-6 * s and abs(np.linalg.norm(nrm) - 1) <= 1e-5, (off, got[2])
        assert box.shape().contains(pos, tol=0.5 * abs(dist) + 2e-6 * s) and through.shape().contains(pos, tol=0.5 * abs(dist) + 2e-6 * s)
        assert I.separation_along(box.shape(), through.shape(), nrm / np.linalg.norm(nrm)) <= dist + 2e-6 * s + 1e-3 * abs(dist)
        _check_single([(box, one_end)], [(-0.002, np.array([0, 0, 1.0]), off + [0.01, 0.005, h[2] - 0.001])], [got[3]], ("box-capsule, one end", off))


def test_cylinder_sphere_designed(gpu):
    r, L, rs = 0.02, 0.03, 0.01
    cases = [
        (("sphere", [rs], [0.017, 0, 0.005]), (-0.003 - rs, [1, 0, 0], [r - 0.5 * (0.003 + rs), 0, 0.005])),            # inside, nearer the side
        (("sphere", [rs], [0.004, 0, 0.028]), (-0.002 - rs, [0, 0, 1], [0.004, 0, L - 0.5 * (0.002 + rs)])),            # inside, nearer the cap
        (("sphere", [rs], [r + 0.003, 0, L + 0.004]), (-0.005, [0.6, 0, 0.8], [r - 0.0025 * 0.6, 0, L - 0.0025 * 0.8])),  # rim
        (("sphere", [rs], [0, -r - 0.006, 0.01]), (-0.004, [0, -1, 0], [0, -r + 0.002, 0.01])),                          # side
    ]
    prs, wants = _local_cases("cylinder", [r, L], TILT, cases)
    _check_single(prs, wants, P.collide("cylinder_sphere", prs), "cylinder-sphere")
    # on the axis beyond the cap (the branch without a radial direction) and exactly touching (no contact): axis-aligned, binary fractions -- exact in fp32
    r, L, rs = 2.0 ** -6, 2.0 ** -5, 2.0 ** -7
    cyl = P.Geom("cylinder", [r, L], np.zeros(3), ID)
    prs = [(cyl, P.Geom("sphere", [rs], [0, 0, L + 2.0 ** -8], ID)), (cyl, P.Geom("sphere", [rs], [r + rs, 0, 2.0 ** -7], ID)), (cyl, P.Geom("sphere", [rs], [0, 0, L + rs], ID))]
    _check_single(prs, [(-(2.0 ** -8), np.array([0, 0, 1.0]), np.array([0, 0, L - 2.0 ** -9])), None, None], P.collide("cylinder_sphere", prs), "cylinder-sphere, exact")


def test_convex_cylinder_designed(gpu):
    """Capsule / box / cylinder against the cylinder (one instantiation serves the tree kernel's tire build and the leap cylinder build): depth to 5e-6 + 2e-3 |depth| (the random test holds it to the measured figure), normal to
    1e-4, the position anywhere on the shared feature."""
    routine, r, L, pen = "convex", 0.02, 0.015, 0.001
    cyl = P.Geom("cylinder", [r, L], np.zeros(3), ID)
    down = np.array([0, 0, -1.0])
    flat_capsule = P.Geom("capsule", [0.005, 0.01], [0.002, 0.001, L + 0.005 - pen], P.axis_angle([0, 1, 0], np.pi / 2))
    end_on = P.Geom("capsule", [0.005, 0.01], [0, 0, L + 0.01 + 0.005 - pen], ID)
    flat_box = P.Geom("box", [0.01, 0.008, 0.005], [0.003, 0.002, L + 0.005 - pen], ID)
    edge_box = P.Geom("box", [0.006, 0.01, 0.006], [r + np.sqrt(2) * 0.006 - pen, 0, 0], P.axis_angle([0, 1, 0], np.pi / 4))
    coaxial = P.Geom("cylinder", [0.012, 0.01], [0, 0, L + 0.01 - pen], ID)
    same = P.Geom("capsule", [0.005, 0.01], np.zeros(3), ID)
    prs = [(flat_capsule, cyl), (end_on, cyl), (flat_box, cyl), (edge_box, cyl), (coaxial, cyl), (same, cyl)]
    got = P.collide(routine, prs)   # (finite, and returned: `collide` asserts both -- all the coincident centres are asked for)
    assert len(got[5]) <= 1
    dtol = 5e-6 + 2e-3 * pen
    top = L - 0.5 * pen

    def one(k, n):
        assert len(got[k]) == 1, (routine, k, got[k])
        dist, pos, nrm = got[k][0]
        assert abs(dist + pen) <= dtol and np.abs(nrm - n).max() <= 1e-4, (routine, k, got[k][0])
        return pos

    p = one(0, down)  # the capsule lying flat on the cap: anywhere along its axis
    assert abs(p[0] - 0.002) <= 0.01 + 2e-6 and abs(p[1] - 0.001) <= 2e-6 + np.sqrt(2 * 0.005 * dtol) and abs(p[2] - top) <= dtol, p
    p = one(1, down)  # end-on along the axis: the support direction runs along the cylinder's axis, which the support function's second orthogonalisation is for
    assert np.abs(p[:2]).max() <= np.sqrt(2 * 0.005 * dtol) and abs(p[2] - top) <= dtol, p
    p = one(2, down)  # the box's face flat on the cap: anywhere in the face (inside the disc)
    assert abs(p[0] - 0.003) <= 0.01 + 2e-6 and abs(p[1] - 0.002) <= 0.008 + 2e-6 and np.hypot(p[0], p[1]) <= r + 2e-6 and abs(p[2] - top) <= dtol, p
    p = one(3, np.array([-1.0, 0, 0]))  # the box's edge across the curved side: the point of the edge nearest the axis
    assert abs(p[0] - (r - 0.5 * pen)) <= dtol and abs(p[1]) <= np.sqrt(2 * r * dtol) and abs(p[2]) <= 2e-6 + dtol, p
    p = one(4, down)  # coaxial cylinders: anywhere on the smaller cap
    assert np.hypot(p[0], p[1]) <= 0.012 + 2e-6 and abs(p[2] - top) <= dtol, p
