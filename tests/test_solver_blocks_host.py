"""The references and generators of `tests/blocks.py` against themselves, before a GPU is involved (tests/test_gpu_solver_blocks.py holds the device to them).

The analytic gradient and Hessian of the cone and pyramid costs against central differences of the COST ALONE; continuity of cost and force across both zone boundaries;
the zone shares of the generator and its redraw rule; the fp32 emulations of the DPP pairing orders against fp64 sums; and the constants of every tolerance as asserted
upper bounds of what the references' fp32 shadows need -- a change of a generator that invalidates a tolerance fails here."""

import numpy as np
import pytest

from tests import blocks as B

LD = np.longdouble  # the cost is evaluated in extended precision: second differences at a step of 1e-5 lose ten digits


def _fd(cost, x, h):
    """Gradient (n, 3) and Hessian (n, 3, 3) of cost(x) by central differences of the cost with steps h (n, 3) and h / 2, Richardson-extrapolated to fourth order."""
    n = x.shape[0]

    def at(hh):
        e = np.eye(3, dtype=LD)[None] * hh[:, None, :]  # (n, 3, 3): row i is the step along i
        g, H = np.zeros((n, 3), LD), np.zeros((n, 3, 3), LD)
        for i in range(3):
            g[:, i] = (cost(x + e[:, i]) - cost(x - e[:, i])) / (2 * hh[:, i])
            for j in range(i + 1):
                H[:, i, j] = (cost(x + e[:, i] + e[:, j]) - cost(x + e[:, i] - e[:, j]) - cost(x - e[:, i] + e[:, j]) + cost(x - e[:, i] - e[:, j])) / (4 * hh[:, i] * hh[:, j])
                H[:, j, i] = H[:, i, j]
        return g, H

    (g1, H1), (g2, H2) = at(h.astype(LD)), at(h.astype(LD) / 2)
    return ((4 * g2 - g1) / 3).astype(np.float64), ((4 * H2 - H1) / 3).astype(np.float64)


def _packed(H):
    return np.stack([H[:, 0, 0], H[:, 1, 0], H[:, 1, 1], H[:, 2, 0], H[:, 2, 1], H[:, 2, 2]], 1)


def _rel(a, b):
    """max |a - b| per case over the case's max |b| (0 / 0 is 0)."""
    a, b = a.reshape(len(a), -1), b.reshape(len(b), -1)
    err, mag = np.abs(a - b).max(1), np.abs(b).max(1)
    return np.where(err == 0, 0.0, err / np.where(mag > 0, mag, 1.0))


def test_cone_gradient_and_hessian_are_the_cost_s_central_differences():
    c = B.cone_cases()
    r = B.cone_ref(c)
    z = r["zone"]
    N, T = B.cone_NT(c)
    # a step of 1e-5 of the case's own scale: the zone test moves by at most 6e-5 (|N| + T), inside the margin of 1e-4 every case has; the zone is held fixed all the same
    h = np.repeat((1e-5 * (np.abs(N) + T) / np.maximum(c["mu"], c["fri"]))[:, None], 3, 1)
    cost = lambda x: B.cone_cost(x, c["D"], c["Dm"], c["mu"], c["fri"], LD, zone=z)[0]  # noqa: E731
    g, H = _fd(cost, c["jar"].astype(LD), h)
    eg, eH = _rel(-r["f"], g), _rel(r["W"], _packed(H))
    print(f"cone: analytic against central differences of the cost, relative: gradient {eg.max():.2e}, Hessian {eH.max():.2e} (per zone: "
          + ", ".join(f"{nm} {eg[z == k].max():.1e} / {eH[z == k].max():.1e}" for nm, k in (("top", B.TOP), ("middle", B.MIDDLE), ("bottom", B.BOTTOM))) + ")")
    assert eg.max() < 1e-7 and eH.max() < 1e-7
    # cone_dir's two scalars are that gradient and Hessian along jp
    Hs = np.zeros((len(z), 3, 3))
    for k, (i, j) in enumerate(((0, 0), (1, 0), (1, 1), (2, 0), (2, 1), (2, 2))):
        Hs[:, i, j] = Hs[:, j, i] = r["W"][:, k]
    d1 = c["d0"][:, 0] - (r["f"] * c["jp"]).sum(1)
    d2 = c["d0"][:, 1] + np.einsum("ni,nij,nj->n", c["jp"], Hs, c["jp"])
    s = r["scale"]
    # (jp' W jp sums products of the size of W's scale, which is larger than the scale of d2 written along the line: the two statements agree to fp64 rounding of that)
    Wmag = np.abs(np.einsum("ni,nij,nj->n", np.abs(c["jp"]), np.abs(Hs), np.abs(c["jp"]))) + np.abs(c["d0"][:, 1])
    assert (np.abs(d1 - r["d1"]) <= 1e-12 * (np.abs(r["f"] * c["jp"]).sum(1) + np.abs(c["d0"][:, 0]) + s["d1"] / B.EPS)).all()
    assert (np.abs(d2 - r["d2"]) <= 1e-12 * (Wmag + s["d2"] / B.EPS)).all()


@pytest.mark.parametrize("through_contact_eval", [False, True])
def test_pyramid_gradient_and_hessian_are_the_cost_s_central_differences(through_contact_eval):
    c = B.pyramid_cases(through_contact_eval=through_contact_eval)
    r = B.pyramid_ref(c)
    j, mu = c["jar"], c["pmu"]
    # The cost is piecewise quadratic, so its central differences are exact for any step that takes no row across 0, up to the rounding of the cost over the step squared.
    # The two tangents' rows may differ by decades in size: each pair's part of the cost is differenced on its own, with steps of a quarter of its nearer row's distance
    # from 0 (no row is nearer than 1e-4 of its size), and the parts are added.
    g, H = np.zeros((len(mu), 3)), np.zeros((len(mu), 3, 3))
    for rows, t in (((0, 1), 1), ((2, 3), 2)):
        m = 0.25 * np.minimum(np.abs(j[:, 0] + mu * j[:, t]), np.abs(j[:, 0] - mu * j[:, t]))
        gp, Hp = _fd(lambda x: B.pyramid_cost(x, c["D"][:, 0], mu, LD, rows), j.astype(LD), np.stack([m, m / mu, m / mu], 1))
        g, H = g + gp, H + Hp
    eg, eH = _rel(-r["f"], g), _rel(r["W"], _packed(H))
    print(f"pyramid: analytic against central differences of the cost, relative: gradient {eg.max():.2e}, Hessian {eH.max():.2e}; active rows 0..4: {np.bincount(r['nact'], minlength=5)}")
    assert eg.max() < 1e-7 and eH.max() < 1e-7
    assert (np.bincount(r["nact"], minlength=5)[[0, 4]] > 0.1 * len(mu)).all(), "all four rows active, and none, are each a tenth of the draws"
    want = {"four rows": 4, "no row": 0, "a row at 0": 3, "a row at 0, none active": 0, "all zero": 0}
    for name, d in B.DESIGNED_PYRAMID.items():
        assert B.pyramid_ref(d)["nact"][0] == want[name], name
    d = B.DESIGNED_PYRAMID["a row at 0"]  # jar_n + mu jar_t1 is exactly 0: that row is inactive, its opposite and both rows of the other tangent are active
    assert (d["jar"][0, 0] + d["pmu"][0] * d["jar"][0, 1]) == 0.0 and (B.pyramid_ref(d)["W"][0] == [3072.0, -512.0, 256.0, 0.0, 0.0, 512.0]).all()


def test_cost_and_force_are_continuous_across_both_zone_boundaries():
    """In exact arithmetic with D1 = D0 impratio, mu = fri / sqrt(impratio), Dm = D0 / (mu^2 (1 + mu^2)): here in fp64, on points ON each boundary, through both zones' statements."""
    rng = np.random.default_rng(7)
    n = 2000
    fri, impratio, D0 = rng.uniform(0.2, 2, n), rng.choice([1.0, 3.0, 10.0], n), 10.0 ** rng.uniform(1, 5, n)
    mu = fri / np.sqrt(impratio)
    jt = rng.standard_normal((n, 2)) * 10.0 ** rng.uniform(-3, 1, (n, 1))
    T = fri * np.linalg.norm(jt, axis=1)
    base = dict(jp=rng.standard_normal((n, 3)), D=np.stack([D0, D0 * impratio, D0 * impratio], 1), Dm=D0 / (mu**2 * (1 + mu**2)), mu=mu, fri=fri, d0=np.zeros((n, 2)))
    for name, j0, zones in (("top", T, (B.TOP, B.MIDDLE)), ("bottom", -T / mu**2, (B.BOTTOM, B.MIDDLE))):
        c = dict(base, jar=np.concatenate([j0[:, None], jt], 1))
        a, b = (B.cone_ref(c, zone=np.full(n, z)) for z in zones)
        A = np.abs(mu * j0) + mu * T  # the middle zone's magnitudes: Dm A^2 for the cost, Dm mu A max(1, fri) for the force, Dm A (|V0| + mu |Vt|) for d1
        mag_f = (b["scale"]["f"] / B.EPS).max(1)
        ds, df, dd = np.abs(a["s"] - b["s"]) / (base["Dm"] * A * A), np.abs(a["f"] - b["f"]).max(1) / mag_f, np.abs(a["d1"] - b["d1"]) / (b["scale"]["d1"] / B.EPS)
        print(f"{name} boundary: jump of s {ds.max():.1e}, of f {df.max():.1e}, of d1 {dd.max():.1e} (relative to the middle zone's magnitudes); W jumps by {np.abs(a['W'] - b['W']).max(1).min():.1e} at least")
        assert ds.max() < 1e-12 and df.max() < 1e-12 and dd.max() < 1e-12
        assert (np.abs(a["W"] - b["W"]).max(1) > 0).all()  # the Hessian does jump: the device may show either side's on a boundary


def test_cone_generator_places_its_draws_and_leaves_no_case_out():
    c = B.cone_cases()
    n = B.N_CASES
    assert all(len(v) == n for v in c.values())
    assert (B.cone_margin(c) >= B.MIN_MARGIN).all()
    assert (np.bincount(c["place"].astype(int)) == [n - n // 3 - n // 6, n // 3, n // 6]).all()
    z = B.cone_zone(c)
    share = np.bincount(z, minlength=3) / n
    rest = np.bincount(z[c["place"] == 0], minlength=3) / (c["place"] == 0).sum()
    print(f"zones top / middle / bottom: {share} of all draws, {rest} of those that fall where they fall; smallest margin {B.cone_margin(c).min():.3e}")
    assert (share >= 0.1).all()
    assert (z == B.cone_zone(c, np.float32)).all(), "with a margin of 1e-4 the fp32 shadow sees every case in the fp64 zone"
    # near a boundary means near it: the placed thirds and sixths lie within 0.1 of theirs
    N, T = B.cone_NT(c)
    assert (np.abs(N - c["mu"] * T)[c["place"] == 1] <= 0.11 * (c["mu"] * T)[c["place"] == 1]).all() and (z[c["place"] == 1] == B.MIDDLE).all()
    assert (np.abs(c["mu"] * N + T)[c["place"] == 2] <= 0.11 * T[c["place"] == 2]).all() and set(z[c["place"] == 2]) == {B.MIDDLE, B.BOTTOM}
    # every input is an fp32 number, and the slot's constants are the fp32 evaluations the kernels make
    rows = B.cone_rows(c)
    m2 = rows[:, 10] * rows[:, 10]
    assert (rows[:, 9] == rows[:, 6] / (m2 * (np.float32(1) + m2))).all() and (rows[:, 7] == rows[:, 8]).all()
    # the designed cases sit where their names say
    want = {"T=0 N>0": B.TOP, "T=0 N<0": B.BOTTOM, "T=0 N=0": B.TOP, "T2 underflows N>0": B.TOP, "T2 underflows N<0": B.BOTTOM, "T2 denormal N>0": B.TOP, "T2 denormal N<0": B.BOTTOM, "empty slot": B.TOP}
    for name, d in B.DESIGNED_CONE.items():
        assert B.cone_zone(d)[0] == want[name], name
    j = B.DESIGNED_CONE["T2 underflows N<0"]["jar"].astype(np.float32)
    assert j[0, 1] != 0 and (j[0, 1] * j[0, 1] + j[0, 2] * j[0, 2]) == 0
    j = B.DESIGNED_CONE["T2 denormal N<0"]["jar"].astype(np.float32)
    assert 0 < j[0, 2] * j[0, 2] < np.finfo(np.float32).tiny
    for name, (d, zones) in B.DESIGNED_BOUNDARY.items():
        N, T = B.cone_NT(d)
        assert (N[0] == d["mu"][0] * T[0]) if zones[0] == B.TOP else (d["mu"][0] * N[0] + T[0] == 0), name
        N32, T32 = B.cone_NT(d, np.float32)
        assert N32[0] == N[0] and T32[0] == T[0], (name, "the boundary is hit in fp32 as well")


def test_impedance_reference():
    def scalar(si, dist):  # the formula tests/test_oracle_contact_facts.py has always used, one case at a time
        d0, d1, width, mid, power = si
        x = min(abs(dist) / width, 1.0)
        y = x if power == 1 else (x**power / mid ** (power - 1) if x <= mid else 1 - (1 - x) ** power / (1 - mid) ** (power - 1))
        return d0 + y * (d1 - d0)

    si, dist, grp = B.impedance_cases()
    ref = B.impedance(si.T, dist)
    live = (si[:, 0] != si[:, 1]) & (si[:, 2] > float(np.float32(1e-15)))
    idx = np.flatnonzero(live)[::37]
    assert max(abs(scalar(si[i], dist[i]) - ref[i]) for i in idx) < 1e-15
    assert (ref[~live] == 0.5 * (si[~live, 0] + si[~live, 1])).all()
    assert isinstance(B.impedance((0.9, 0.95, 0.001, 0.5, 2.0), -3e-4), float) and B.impedance((0.9, 0.95, 0.001, 0.5, 2.0), -3e-4) == pytest.approx(0.9 + 0.05 * 0.18)
    # the two branches meet at the midpoint; symmetric; inside [d0, d1]; every power, midpoint and width edge of the curve is among the cases
    x, mid, p = si[live, 3], si[live, 3], si[live, 4]
    assert np.abs(x**p / mid ** (p - 1) - (1 - (1 - x) ** p / (1 - mid) ** (p - 1))).max() < 1e-12
    lo, hi = np.minimum(si[:, 0], si[:, 1]), np.maximum(si[:, 0], si[:, 1])
    assert ((ref >= lo) & (ref <= hi)).all()
    assert {1.0, 2.0, 1.5, 3.0, 6.0} <= set(si[:, 4]) and {np.float64(np.float32(1e-4)), np.float64(np.float32(0.9999))} <= set(si[:, 3])
    assert {np.float64(np.float32(1e-15)), np.float64(np.float32(2e-15)), 0.0} <= set(si[:, 2]) and (si[:, 0] == si[:, 1]).any() and (si[:, 0] > si[:, 1]).any()
    from judo_amd.models import clamp_solimp

    assert {tuple(np.float32(clamp_solimp(list(s)))) for s in B.model_solimps()} <= {tuple(np.float32(r)) for r in si} and len(B.model_solimps()) >= 3
    for g in np.unique(grp):
        m = grp == g
        d = dist[m]
        assert set(d) == set(-d) and 0.0 in d and np.float64(np.float32(si[m][0, 3]) * (np.float32(si[m][0, 2]) or np.float32(1e-3))) in d
    print(f"impedance: {len(dist)} cases, {len(np.unique(grp))} solimps")


def test_frame_reference_and_cases():
    nrm = B.frame_cases()
    x, y, z, use_z = B.frame_ref(nrm)
    Rm = np.stack([x, y, z], 1)
    assert np.abs(Rm @ np.transpose(Rm, (0, 2, 1)) - np.eye(3)).max() < 1e-14 and (np.linalg.det(Rm) > 0.99).all()
    ln = np.linalg.norm(nrm, axis=1)
    assert ln.min() >= 0.0999 and ln.max() <= 10.001 and 0.2 < use_z.mean() < 0.8
    amb = B.frame_ambiguous(nrm)
    xy = np.abs(nrm[:, 1]) / ln
    print(f"make_frame: {len(nrm)} normals, {amb.sum()} within 4 eps32 of |x_y| = 0.5, of which {(xy[amb] > 0.5).sum()} above; nearest clear ones {np.abs(xy[~amb] - 0.5).min() / B.EPS:.1f} eps32 away")
    assert amb.sum() >= 64 and (xy[amb] > 0.5).any() and (xy[amb] < 0.5).any() and np.abs(xy[~amb] - 0.5).min() < 64 * B.EPS
    for a in np.concatenate([np.eye(3), -np.eye(3)]):
        assert (np.abs(nrm / ln[:, None] - a).max(1) < 1e-7).any()


def test_cholesky_cases_and_shadow():
    for N in (3, 4, 6, 7, 9):
        A, b, kind = B.spd_cases(N, n=256)
        assert (A == np.transpose(A, (0, 2, 1))).all() and (A == B.f32(A)).all() and set(kind) == {0, 1, 2} and (kind == 2).sum() == 4 and (kind[-4:] == 2).all()
        ev = np.linalg.eigvalsh(A)
        ok = kind != 2
        cond = ev[ok, -1] / ev[ok, 0]
        assert ev[ok, 0].min() > 0 and cond.min() < 3 and 3e3 < cond.max() < 2e5 and ev[ok, -1].min() < 1e-2 and ev[ok, -1].max() > 1e2
        assert abs(ev[-1, 0]) < 1e-12 * ev[-1, -1] and abs(ev[-2, 0]) < 1e-12 and abs(ev[-4, 0]) < 1e-12 * ev[-4, -1] and ev[-3, 0] < -0.999, "the last four have an eigenvalue at or below 0"
        # the pivots that must be clamped are exactly 0 and -1 in the fp32 shadow (they are sums of exact zeros: no contraction or order can move them), so the clamp
        # fmaxf(d, 1e-30f) is taken and the reciprocal root is that of 1e-30; the [[4, 4], [4, 4]] block's second pivot is 0 as well where the root of 4 is exact
        Ls, ys, xs, piv, inv = B.chol_shadow(A, b, pivots=True)
        for i, pp in B.clamped_pivots(N, len(b)).items():
            assert piv[i, pp] in (0.0, -1.0) and piv[i, pp] <= 1e-30 and abs(inv[i, pp] / B.RSQ_CLAMP - 1) <= B.EPS, (N, i, piv[i])
            assert (np.delete(piv[i], pp) > 1e-30).all(), "that pivot alone"
        assert piv[-3, N // 2] == -1.0 and piv[-4, N // 2] == 0.0 and piv[-2, 1] == 0.0
        assert np.isfinite(Ls[-4:]).all() and np.isfinite(ys[-4:]).all() and np.isfinite(xs[-4:]).all()
        blk = A[kind == 1]
        assert (blk[:, N // 2:, : N // 2] == 0).all() and (np.abs(A[kind == 0][:, N - 1, 0]) > 0).all()
        L, y, x = B.chol_shadow(A[ok], b[ok], np.float64)  # the shadow's statements are a Cholesky: in fp64 they are numpy's
        assert np.abs(L - np.linalg.cholesky(A[ok])).max() / np.abs(L).max() < 1e-9
        assert np.abs(x - np.linalg.solve(A[ok], b[ok][:, :, None])[:, :, 0]).max() / np.abs(x).max() < 1e-8
        assert np.abs(B.unpack(B.pack(A), N) - np.tril(A)).max() == 0


def test_butterfly_emulations_sum_what_they_say():
    v, sv, iv, special = B.row_cases()
    assert v.shape[0] % 4 == 0 and special.sum() >= 32 and all(special[r: r + 4].sum() <= 1 for r in range(0, len(special), 4))
    assert np.isnan(v[special]).any() and np.isposinf(v[special]).any() and np.isneginf(v[special]).any() and (np.abs(v[special]) == np.float32(3e38)).any()
    sub = np.abs(v) < np.finfo(np.float32).tiny
    assert (sub & (v != 0)).sum() > 200 and (iv == -2**31).any() and (iv < 0).any()
    ok = ~special
    x, X = v[ok].astype(np.float64), sv[ok].astype(np.float64)
    tol = lambda a: 4 * B.EPS * np.abs(a).sum(-1, keepdims=True)  # noqa: E731  (at most four additions deep, half an eps32 of the partial sums each)
    g, c, q, qs = (f(v[ok]).astype(np.float64) for f in (B.emu_gsum, B.emu_csum, B.emu_qsum4, B.emu_qsum4_same))
    assert (np.abs(g - x.sum(1, keepdims=True)) <= tol(x)).all() and (g == g[:, :1]).all()
    quads = x.reshape(-1, 4, 4)
    assert (np.abs(c.reshape(-1, 4, 4) - quads.sum(2, keepdims=True)) <= tol(quads)).all() and (c.reshape(-1, 4, 4) == c.reshape(-1, 4, 4)[:, :, :1]).all()
    cols = np.transpose(quads, (0, 2, 1))  # [row, position in the quad, quad]
    for e, same in ((q, False), (qs, True)):
        e = np.transpose(e.reshape(-1, 4, 4), (0, 2, 1))
        assert (np.abs(e - cols.sum(2, keepdims=True)) <= tol(cols)).all()
        if same:
            assert (e == e[:, :, :1]).all()
    assert (np.transpose(q.reshape(-1, 4, 4), (0, 2, 1)) != np.transpose(q.reshape(-1, 4, 4), (0, 2, 1))[:, :, :1]).any(), "qsum4's lanes do differ: the pairing orders are four associations"
    # exact cancellations come out as exact zeros
    assert (B.emu_gsum(v[:64]) == 0).all()
    s = B.emu_row_scatter16(sv[ok]).astype(np.float64)
    assert (np.abs(s - X.sum(1)) <= 4 * B.EPS * np.abs(X).sum(1)).all(), "lane l holds the sum over the row's lanes of v[l]"
    # a row with a NaN sums to NaN in every lane, in the emulation as in IEEE
    nan_rows = np.isnan(v).any(1)
    assert nan_rows.sum() >= 8 and np.isnan(B.emu_gsum(v[nan_rows])).all()


def test_tolerance_constants_cover_four_times_the_shadow():
    needs = B.shadow_needs()
    assert set(needs) == set(B.C_TOL)
    for name, (c, recorded) in B.C_TOL.items():
        print(f"{name:22s} constant {c:3d}   shadow's need {needs[name]:.3f} on the tests' cases, {recorded} on 8 x 4096 draws")
        if name in B.FIXED_BOUND:
            assert needs[name] <= recorded * 1.001 <= c, name
        else:
            assert needs[name] <= recorded * 1.001 and c == B.constant(recorded) and 4 * needs[name] <= c, name
