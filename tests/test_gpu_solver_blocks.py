"""The solver's device building blocks alone against fp64 references (tests/blocks.py, judo_amd/csrc/jh_xcheck_blocks.hip): the cost, force and Hessian block of one
contact (`cone_eval`, `cone_top` + `cone_below`, `cone_dir`, `pyramid_eval`, `contact_eval`), `impedance`, `make_frame`, the packed Cholesky and its solves
(`chol_packed` / `fwd_packed` / `bwd_packed` <3, 6, 7>, `chol4` / `fwd4` / `bwd4`, `arm_chol_solve` against `chol_solve<9>`) and the row-local DPP reductions and
broadcasts.  The physics tests reach all of these only through whole steps, where a wrong Hessian block costs Newton iterations and nothing else, and where the branch
a state takes is neither controlled nor counted.

Every bound is a running-error scale from the fp64 reference times a constant of `blocks.C_TOL`: 4 times what the reference's own fp32 shadow needs, a power of two,
set without the device (tests/test_solver_blocks_host.py asserts the shadow's side).  Three bounds are fixed by reasoning instead and named in `blocks.FIXED_BOUND`:
orthonormal rows (8 eps32), the sums against fp64 (4 eps32 sum |v|), chol4's L_pp inv_p (4 eps32).  Each comparison is recorded as the USED SHARE of its scale -- `bounded(what, need,
constant)` -- and printed before it is asserted.  A scale of 0 (the top zone's zeros, the bottom zone's W = D) asks for the exact value.

Bit claims, all within the one translation unit of the test kernel.  HELD: csum, gsum and qsum4_same are the same bits in every lane of their group and, with qsum4
and row_scatter16, the bits of the documented pairing order emulated in numpy fp32; arm_chol_solve's x is the same bits in all sixteen lanes; nothing crosses from one
DPP row of a wave into another; imp(dist) == imp(-dist).  NOT HELD, comments corrected, pairs held to the tolerance instead: cone_top + cone_below against cone_eval (W),
arm_chol_solve against chol_solve<9> -- contraction into fma is the compiler's choice per inlined copy.

Found here and fixed in jh_engine_common.h: a squared tangential part T2 that is a DENORMAL fp32 number (a tangential |jar| of 4e-23 to 1e-19 at fri = 1) went through
v_rsq_f32, which flushes it to zero and returns infinity; T = T2 * inf made cone_eval return s = inf and NaN forces, and cone_dir NaN, where the reference has the
T == 0 case ("T2 denormal N>0": s = 0, f = 0 expected, inf / NaN before the fix).  Such a T2 now counts as 0 (CONE_T2_MIN).
"""

import functools

import numpy as np
import pytest

from tests import blocks as B
from tests.conftest import bounded

pytestmark = pytest.mark.gpu
ZONES = (("top", B.TOP), ("middle", B.MIDDLE), ("bottom", B.BOTTOM))


def _hold(what, got, ref, scale, cname, mask=None):
    """|got - ref| <= constant * scale everywhere (exactly equal where there is no constant or the scale is 0); prints the used share first."""
    need = B.need(got, ref, scale, mask)
    c = B.c_of(cname) if cname else 0
    print(f"{what}: needs {need:.3f} of its scale, constant {c}")
    return bounded(what, need, c)


def _cone_out(out):
    o = out.astype(np.float64)
    return dict(s=o[:, 0], f=o[:, 1:4], W=o[:, 4:10], top=out[:, 10], f2=out[:, 11:14], W2=out[:, 14:20], d1=o[:, 20], d2=o[:, 21])


def _cone_needs(tag, got, r, family="cone", keys=("s", "f", "W", "d1", "d2")):
    """[(what, need, constant)] of the device's cone outputs against the reference `r`, zone by zone.  Top: exact zeros (cone_dir leaves what it was given).  Bottom: W = D exactly."""
    res = []
    for zname, z in ZONES:
        m = r["zone"] == z
        if not m.any():
            continue
        for k in keys:
            exact = zname == "top" or (zname == "bottom" and k == "W")
            name = None if exact else f"{'cone_dir' if k in ('d1', 'd2') else 'cone' if zname == 'bottom' else family} {zname} {k}"
            res.append((f"{tag}: {zname} zone ({m.sum()} cases), {k}", B.need(got[k], r[k], r["scale"][k], m), B.c_of(name) if name else 0))
    return res


def _record(needs):
    """Prints and records each (what, need, constant); True where all are within."""
    ok = True
    for what, need, c in needs:
        print(f"{what}: needs {need:.3f} of its scale, constant {c}")
        ok &= bounded(what, need, c)
    return ok


def _hold_cone(tag, got, r, family="cone", keys=("s", "f", "W", "d1", "d2")):
    return _record(_cone_needs(tag, got, r, family, keys))


@functools.lru_cache(maxsize=None)
def _cone_run():
    c = B.cone_cases()
    return c, B.cone_ref(c), B.launch("cone", B.cone_rows(c))


def test_cone_eval_and_cone_dir_random(gpu):
    c, r, out = _cone_run()
    got = _cone_out(out)
    assert np.isfinite(out[:, :11]).all() and np.isfinite(out[:, 20:22]).all()
    assert _hold_cone("cone_eval / cone_dir", got, r)


def test_cone_top_and_cone_below_against_cone_eval(gpu):
    """cone_top is cone_eval's zone test, and cone_below its bottom / middle part "expression for expression".  jh_engine_common.h also claimed "(same bits)": that does
    NOT hold -- on an MI355X the test kernel's two inlined copies gave the same f everywhere and a W that differs in its last bits in 2 385 of 21 942 entries (the compiler
    contracts each copy into fma on its own); the comment is corrected, the count is printed, and cone_below is held to the reference with cone_eval's own constants."""
    c, r, out = _cone_run()
    d = B.concat(list(B.DESIGNED_CONE.values()) + [v[0] for v in B.DESIGNED_BOUNDARY.values()])
    out = np.concatenate([out, B.launch("cone", B.cone_rows(d))])
    zone = np.concatenate([r["zone"], B.cone_zone(d)])
    top = out[:, 10] == 1.0
    assert ((out[:, 10] == 1.0) | (out[:, 10] == 0.0)).all()
    n_rand = len(r["zone"])
    assert (top[:n_rand] == (zone[:n_rand] == B.TOP)).all(), "cone_top is the reference's top zone on every case with a margin"
    # cone_eval's own zone shows in its W: W[0] is mu Dm mu or D0, both positive, below the top zone (the all-zero empty slot has W = 0 and is top)
    eval_top = (out[:, 4] == 0) & (out[:, 0] == 0)
    assert (top == eval_top).all(), "cone_top returns true exactly where cone_eval returns the top zone"
    assert np.isnan(out[top][:, 11:20]).all(), "cone_below is not called where cone_top holds: the kernel wrote nothing there"
    below = ~top
    same_f, same_W = B.same_bits(out[below, 1:4], out[below, 11:14]), B.same_bits(out[below, 4:10], out[below, 14:20])
    print(f"cone_top + cone_below against cone_eval on {below.sum()} cases below the top zone: f differs in {(~same_f).sum()} of {same_f.size} entries, W in {(~same_W).sum()} of {same_W.size}")
    m = below[:n_rand]
    sub = {k: v[m] for k, v in r.items() if k != "scale"}
    sub["scale"] = {k: v[m] for k, v in r["scale"].items()}
    o = out[:n_rand][m].astype(np.float64)
    assert np.isfinite(o[:, 11:20]).all()
    assert _hold_cone("cone_below", dict(f=o[:, 11:14], W=o[:, 14:20]), sub, keys=("f", "W"))


def test_cone_designed_cases(gpu):
    names = list(B.DESIGNED_CONE)
    d = B.concat([B.DESIGNED_CONE[k] for k in names])
    out = B.launch("cone", B.cone_rows(d))
    got, r = _cone_out(out), B.cone_ref(d)
    for i, nm in enumerate(names):
        print(f"{nm}: zone {r['zone'][i]}, device s {out[i, 0]!r} f {out[i, 1:4]} W {out[i, 4:10]} top {out[i, 10]} d {out[i, 20:22]}; reference s {r['s'][i]!r} f {r['f'][i]} d {r['d1'][i]!r} {r['d2'][i]!r}")
    assert np.isfinite(out[:, :11]).all() and np.isfinite(out[:, 20:22]).all(), "no NaN or infinity out of a finite input"
    assert _hold_cone("designed", got, r)
    e = names.index("empty slot")  # "an empty slot is all zeros ... its cone test reads `top`, its terms are zero" (jh_engine_v5.hip)
    assert (out[e, :10] == 0).all() and out[e, 10] == 1.0 and out[e, 20] == np.float32(0.5) and out[e, 21] == np.float32(-0.25)


@pytest.mark.parametrize("name", list(B.DESIGNED_BOUNDARY))
def test_cone_exactly_on_a_zone_boundary(gpu, name):
    """s, f and d1 are continuous across a boundary and stay under the tolerance; W and d2 jump there: either adjacent zone's."""
    d, zones = B.DESIGNED_BOUNDARY[name]
    out = B.launch("cone", B.cone_rows(d))
    got = _cone_out(out)
    assert np.isfinite(out[:, :11]).all() and np.isfinite(out[:, 20:22]).all()
    sides = []
    for z in zones:
        r = B.cone_ref(d, zone=np.full(1, z))
        zn = {B.TOP: "top", B.MIDDLE: "middle", B.BOTTOM: "bottom"}[z]
        print(f"{name}, as {zn}: device s {out[0, 0]!r} f {out[0, 1:4]} W {out[0, 4:10]} d {out[0, 20:22]}; reference s {r['s'][0]!r} f {r['f'][0]} W {r['W'][0]} d {r['d1'][0]!r} {r['d2'][0]!r}")
        sides.append(_cone_needs(f"{name}, as {zn}", got, r))
    # the side the device took is the one it is held to and the only one recorded: the first whose every bound holds, or, if neither does, the nearer one
    excess = [max((n - c if c else (0.0 if n == 0 else np.inf)) for _, n, c in side) for side in sides]
    assert _record(sides[int(np.argmin(excess))])


@functools.lru_cache(maxsize=None)
def _pyramid_designed(through):
    d = B.concat(list(B.DESIGNED_PYRAMID.values()))
    return d, B.launch("contact" if through else "pyramid", B.pyramid_rows(d, through))


def _hold_pyramid(tag, out, r):
    o = out.astype(np.float64)
    assert np.isfinite(out[:, :10]).all()
    ok = True
    for k, sl in (("s", slice(0, 1)), ("f", slice(1, 4)), ("W", slice(4, 10))):
        ok &= _hold(f"{tag}: {k}", o[:, sl].reshape(r[k].shape), r[k], r["scale"][k], f"pyramid {k}")
    return ok


@pytest.mark.parametrize("through_contact_eval", [False, True], ids=["pyramid_eval", "contact_eval"])
def test_pyramid_eval(gpu, through_contact_eval):
    """The four one-sided rows 1/2 D min(0, jar_n +- mu jar_t)^2 and their derivatives; a row at exactly 0 is inactive.  Through contact_eval (cone 0 and 2: anything but 1)
    the pyramid's mu is the slot's `fri`."""
    fam = "contact" if through_contact_eval else "pyramid"
    c = B.pyramid_cases(through_contact_eval=through_contact_eval)
    if through_contact_eval:
        c["cone"] = np.where(np.arange(len(c["mu"])) % 2, 2.0, 0.0)
    r = B.pyramid_ref(c)
    print(f"active rows 0..4: {np.bincount(r['nact'], minlength=5)}")
    assert _hold_pyramid(f"{fam}, random", B.launch(fam, B.pyramid_rows(c, through_contact_eval)), r)
    d, out = _pyramid_designed(through_contact_eval)
    rd = B.pyramid_ref(d)
    for i, nm in enumerate(B.DESIGNED_PYRAMID):
        print(f"{nm}: {rd['nact'][i]} active rows, device s {out[i, 0]!r} f {out[i, 1:4]} W {out[i, 4:10]}; reference s {rd['s'][i]!r} f {rd['f'][i]} W {rd['W'][i]}")
    assert _hold_pyramid(f"{fam}, designed", out, rd)
    assert (out[:, 8] == 0).all(), "the two tangents' rows share no weight: W21 is 0"


def test_contact_eval_elliptic(gpu):
    """cone == 1: cone_eval with Dm = D0 / (mu^2 (1 + mu^2)) from __frcp_rn."""
    c = B.cone_cases()
    r = B.contact_ref(c)
    out = B.launch("contact", B.cone_rows(c))
    assert np.isfinite(out[:, :10]).all()
    assert _hold_cone("contact_eval, cone 1", _cone_out(out), r, family="contact", keys=("s", "f", "W"))


def test_impedance(gpu):
    si, dist, grp = B.impedance_cases()
    rows = np.zeros((len(dist), B.IN_F["impedance"]), dtype=np.float32)
    rows[:, :5], rows[:, 5] = si, dist
    got = B.launch("impedance", rows)[:, 0]
    ref = B.impedance(si.T, dist)
    c = B.c_of("impedance")
    err = np.abs(got.astype(np.float64) - ref) / B.EPS
    worst = int(err.argmax())
    print(f"impedance: {len(dist)} cases of {len(np.unique(grp))} solimps; largest error {err.max():.3f} eps32 (constant {c}) at solimp {si[worst]} dist {dist[worst]!r}; by power: "
          + ", ".join(f"{p:g}: {err[si[:, 4] == p].max():.2f}" for p in np.unique(si[:, 4])))
    assert np.isfinite(got).all()
    assert bounded("impedance: |device - fp64| in eps32", err.max(), c)
    lo, hi = np.minimum(si[:, 0], si[:, 1]), np.maximum(si[:, 0], si[:, 1])
    outside = np.maximum(lo - got, got - hi).max() / B.EPS
    back, sym = 0.0, True
    for g in np.unique(grp):
        m = np.flatnonzero(grp == g)  # (dist ascending and symmetric about 0)
        assert (dist[m] == -dist[m][::-1]).all()
        sym &= bool((got[m].view(np.uint32) == got[m][::-1].view(np.uint32)).all())
        h = m[dist[m] >= 0]
        step = np.diff(got[h].astype(np.float64)) * np.sign(si[m[0], 1] - si[m[0], 0])
        back = max(back, float(-step.min()) / B.EPS)
    print(f"impedance: outside [min(d0, d1), max(d0, d1)] by {outside:.3f} eps32 at the most, steps back along |dist| by {back:.3f} eps32 at the most; imp(dist) == imp(-dist) to the bit: {sym}")
    assert sym, "imp(dist) == imp(-dist) to the bit"
    assert bounded("impedance: outside [min(d0, d1), max(d0, d1)], eps32", outside, c) and bounded("impedance: not monotonic in |dist|, eps32", back, c)
    # the mean where d0 == d1 or the width is at most 1e-15, whatever dist
    flat = (si[:, 0] == si[:, 1]) | (si[:, 2] <= float(np.float32(1e-15)))
    assert flat.any() and (got[flat] == (np.float32(0.5) * (si[flat, 0].astype(np.float32) + si[flat, 1].astype(np.float32)))).all()


def test_make_frame(gpu):
    nrm = B.frame_cases()
    rows = np.zeros((len(nrm), B.IN_F["frame"]), dtype=np.float32)
    rows[:, :3] = nrm
    out = B.launch("frame", rows).astype(np.float64)
    assert np.isfinite(out).all()
    fn = B.frame_needs(nrm, out[:, 0:3], out[:, 3:6], out[:, 6:9])
    amb = B.frame_ambiguous(nrm)
    print(f"make_frame: {len(nrm)} normals, {amb.sum()} of them within 4 eps32 of |x_y| = 0.5, where either tangent is right; elsewhere the choice is the reference's on {(fn['chosen_ok'] & ~amb).sum()} of {(~amb).sum()}")
    for k in ("y", "z", "parallel", "cross", "orthonormal"):
        print(f"make_frame: {k} needs {fn[k].max():.3f} eps32, constant {B.c_of('frame ' + k)}")
    assert fn["chosen_ok"].all(), "the tangent is built from the reference's axis wherever |x_y| is clear of 0.5"
    assert all([bounded(f"make_frame: {k}, eps32", fn[k].max(), B.c_of("frame " + k)) for k in ("y", "z", "parallel", "cross", "orthonormal")])


@pytest.mark.parametrize("N", [3, 6, 7, 4], ids=["chol_packed<3>", "chol_packed<6>", "chol_packed<7>", "chol4"])
def test_packed_cholesky_and_its_solves(gpu, N):
    """Residuals in fp64 (they do not grow with the condition number): ||L L' - A||_max <= c N eps ||A||_max with the diagonal slots holding 1 / L_pp, the forward solve
    ||L y - b||_inf <= c N eps ||L||_inf ||y||_inf, both solves ||A x - b||_inf <= c N eps ||A||_inf ||x||_inf.  N = 3, 6, 7 are all the shipped kernels instantiate
    (jh_engine_v4.hip); 4 is chol4 / fwd4 / bwd4, which keeps the diagonal and its reciprocal apart.  Four cases have a pivot at or below zero; two of them exactly, and
    there the clamped slot must hold rsq(1e-30)."""
    A, b, kind = B.spd_cases(N)
    n = len(b)
    T = N * (N + 1) // 2
    if N == 4:
        rows = np.zeros((n, B.IN_F["chol4"]), dtype=np.float32)
        rows[:, :T], rows[:, 10:14] = B.pack(A), b
        out = B.launch("chol4", rows)
        L, inv, y, x = B.unpack(out[:, :T].astype(np.float64), 4), out[:, 10:14].astype(np.float64), out[:, 14:18], out[:, 18:22]
        d = np.einsum("nii->ni", L)
        one = np.abs(d * inv - 1)[kind != 2].max() / B.EPS
        print(f"chol4: |L_pp * inv_p - 1| {one:.3f} eps32")
        assert bounded("chol4: |L_pp inv_p - 1|, eps32", one, B.c_of("chol4 diagonal"))  # (a fixed bound, blocks.FIXED_BOUND)
        slot = inv
    else:
        rows = np.zeros((n, B.IN_F[f"chol{N}"]), dtype=np.float32)
        rows[:, :T], rows[:, 28:28 + N] = B.pack(A), b
        out = B.launch(f"chol{N}", rows)
        L, y, x = B.unpack(out[:, :T].astype(np.float64), N), out[:, 28:28 + N], out[:, 35:35 + N]
        i = np.arange(N)
        with np.errstate(all="ignore"):
            slot = L[:, i, i].copy()
            L[:, i, i] = 1.0 / L[:, i, i]  # the diagonal slots hold 1 / L_pp
    written = np.concatenate([out[:, :T], y, x], 1)
    assert np.isfinite(written).all(), "finite everywhere, the four cases with a pivot at or below zero included"
    # the clamp fmaxf(d, 1e-30f) is TAKEN: a pivot that is exactly 0 (row and column all zero) and one that is exactly -1 come out as v_rsq(1e-30), to its 1 ulp
    for i, pp in B.clamped_pivots(N, n).items():
        print(f"N = {N}, case {i - n}: pivot {pp}'s reciprocal root {slot[i, pp]!r}, rsq(1e-30) = {B.RSQ_CLAMP!r}; the others {np.delete(slot[i], pp)}")
        assert abs(slot[i, pp] / B.RSQ_CLAMP - 1) <= B.EPS and (np.delete(slot[i], pp) < 1e6).all(), (N, i, slot[i])
    print(f"N = {N}: the [[4, 4], [4, 4]] block's second pivot gives {slot[n - 2, 1]!r} (rsq(1e-30) where v_rsq(4) is exactly 0.5), B B' of rank N - 1 gives {slot[n - 1]}")
    ok = kind != 2
    fac, fwd, sol = (v[ok] for v in B.chol_needs(A, b, L, y, x))
    for k, v in (("factor", fac), ("fwd", fwd), ("solve", sol)):
        print(f"N = {N}: {k} residual needs {v.max():.3f} of N eps32 x norms, constant {B.c_of('chol ' + k)}; block-diagonal alone {v[kind[ok] == 1].max():.3f}")
    assert all([bounded(f"N = {N}: {k} residual over N eps32 x norms", v.max(), B.c_of("chol " + k)) for k, v in (("factor", fac), ("fwd", fwd), ("solve", sol))])


def test_arm_chol_solve(gpu):
    """Four different systems per wave.  x is the same bits in all sixteen lanes of a row ("every lane gets x") and solves the system, as chol_solve<9>'s does.  The
    comment also claimed chol_solve<9>'s bits: that does NOT hold -- on an MI355X about two entries in three differ (100 160 of 147 456 on these systems).  arm_chol_solve subtracts with explicit fma;
    chol_solve's `s -= a * b` are contracted as the compiler sees fit, and in the test kernel it packs the multiplies in pairs (64 v_pk_mul_f32) and leaves 77 subtractions
    apart.  The comment is corrected, the count is printed, and both routines are held to the same residual."""
    A, b, kind = B.spd_cases(9, n=1024)
    out = B.launch("arm", B.arm_rows(A, b)).reshape(len(b), 16, B.OUT_F["arm"])
    assert np.isfinite(out).all()
    x, xr = out[:, :, 0:9], out[:, :, 9:18]
    lanes = B.same_bits(x, x[:, :1, :]).all((1, 2))
    ref_lanes = B.same_bits(xr, xr[:, :1, :]).all((1, 2))
    bits = B.same_bits(x, xr)
    ok = kind != 2
    zero = np.zeros_like(b)
    _, _, sol = B.chol_needs(A, b, np.zeros_like(A) + np.eye(9), zero + 1, x[:, 15, :])
    _, _, sol_ref = B.chol_needs(A, b, np.zeros_like(A) + np.eye(9), zero + 1, xr[:, 0, :])
    print(f"arm_chol_solve: {len(b)} systems; x the same bits in all 16 lanes: {lanes.sum()}; solve residual needs {sol[ok].max():.3f} (chol_solve<9>: {sol_ref[ok].max():.3f}), constant {B.c_of('chol solve')}; "
          f"entries whose bits are not chol_solve<9>'s: {(~bits).sum()} of {bits.size}")
    assert lanes.all() and ref_lanes.all()
    assert bounded("arm_chol_solve: solve residual over N eps32 x norms", sol[ok].max(), B.c_of("chol solve"))
    assert bounded("chol_solve<9>: solve residual over N eps32 x norms", sol_ref[ok].max(), B.c_of("chol solve"))


@functools.lru_cache(maxsize=None)
def _row_run():
    """One launch of two copies of the rows: as they are, and with every special row (NaN, +-inf, 3e38) replaced by an ordinary one."""
    v, sv, iv, special = B.row_cases()
    cv, csv = v.copy(), sv.copy()
    cv[special], csv[special] = v[:special.sum()], sv[:special.sum()]
    R = len(v)
    out = B.launch("row", np.concatenate([B.row_rows(v, sv, iv), B.row_rows(cv, csv, iv)])).reshape(2, R, 16, B.OUT_F["row"])
    return v, sv, iv, special, out[0], out[1]


def test_row_sums_are_the_documented_pairing_orders_bit_for_bit(gpu):
    v, sv, iv, special, out, _ = _row_run()
    for k, (name, emu) in enumerate((("csum", B.emu_csum), ("gsum", B.emu_gsum), ("qsum4", B.emu_qsum4), ("qsum4_same", B.emu_qsum4_same))):
        same = B.same_bits(out[:, :, k], emu(v))
        print(f"{name}: {(~same).sum()} of {same.size} lanes differ from the fp32 emulation of its pairing order (rows that differ: {np.flatnonzero(~same.all(1))[:8]})")
        assert same.all(), name
    same = B.same_bits(out[:, :, 4], B.emu_row_scatter16(sv))
    print(f"row_scatter16: {(~same).sum()} of {same.size} lanes differ from the emulation of its four select-and-add levels")
    assert same.all()
    # the same bits in every lane of the group: the quad (csum), the row (gsum), the lanes l, l + 4, l + 8, l + 12 (qsum4_same)
    q = lambda a: a.reshape(-1, 4, 4)  # noqa: E731
    assert B.same_bits(q(out[:, :, 0]), q(out[:, :, 0])[:, :, :1]).all(), "csum is bit-identical in the four lanes of a quad"
    assert B.same_bits(out[:, :, 1], out[:, :1, 1]).all(), "gsum is bit-identical in the sixteen lanes of a row"
    assert B.same_bits(q(out[:, :, 3]), q(out[:, :, 3])[:, :1, :]).all(), "qsum4_same is bit-identical in its four lanes"
    # against the fp64 sums, on the rows that hold numbers.  qsum4's lanes may differ (its comment says so): each is within 4 eps32 sum |v|.
    ok = ~special
    x = v[ok].astype(np.float64)
    cols = np.transpose(q(x), (0, 2, 1))
    got = np.transpose(q(out[ok][:, :, 2].astype(np.float64)), (0, 2, 1))
    need = (np.abs(got - cols.sum(2, keepdims=True)) / np.maximum(B.EPS * np.abs(cols).sum(2, keepdims=True), 1e-300)).max()
    print(f"qsum4 against the fp64 sum: {need:.3f} eps32 sum |v|")
    assert bounded("qsum4 against the fp64 sum, eps32 sum |v|", need, B.c_of("row sums"))  # (a fixed bound, blocks.FIXED_BOUND)
    need = (np.abs(out[ok][:, :, 1].astype(np.float64) - x.sum(1, keepdims=True)) / (B.EPS * np.abs(x).sum(1, keepdims=True))).max()
    assert bounded("gsum against the fp64 sum, eps32 sum |v|", need, B.c_of("row sums"))
    X = sv[ok].astype(np.float64)
    need = (np.abs(out[ok][:, :, 4].astype(np.float64) - X.sum(1)) / (B.EPS * np.abs(X).sum(1))).max()
    print(f"row_scatter16: lane l against the fp64 sum over the row of v[l]: {need:.3f} eps32 sum |v|")
    assert bounded("row_scatter16 against the fp64 sums, eps32 sum |v|", need, B.c_of("row sums"))


def test_row_min_or_and_broadcasts(gpu):
    v, sv, iv, special, out, _ = _row_run()
    bits = out.view(np.uint32)
    assert (bits[:, :, 6].view(np.int32) == np.bitwise_or.reduce(iv, axis=1)[:, None]).all(), "gor: the OR over the row, the sign bit included"
    assert (np.bitwise_or.reduce(iv, axis=1) < 0).any() and (iv[160:192].min(1) == -2**31).all() and (bits[160:192, :, 6] == 0x80000000).all()
    assert (bits[:, :, 7].view(np.int32) == iv.min(1)[:, None]).all(), "gmini: the signed minimum over the row, INT_MIN included"
    # gmin is fminf over the row: it IGNORES a NaN (np.fmin does the same) and is a NaN only where the whole row is
    with np.errstate(all="ignore"):
        want = np.fmin.reduce(v, axis=1)[:, None]
    g = out[:, :, 5]
    assert ((g == want) | (np.isnan(g) & np.isnan(want))).all()
    some_nan = np.isnan(v).any(1)
    assert (some_nan & ~np.isnan(want[:, 0])).any() and np.isnan(want).any(), "rows with a NaN among numbers, and a row of NaNs, are both here"
    lane = np.arange(16)
    for j in range(4):
        assert (bits[:, :, 8 + j] == v.view(np.uint32)[:, (lane & ~3) + j]).all(), f"quad_get(v, {j})"
    for N in range(16):
        assert (bits[:, :, 12 + N] == v.view(np.uint32)[:, N: N + 1]).all(), f"row_bcast<{N}>"


def test_nothing_crosses_from_one_row_of_a_wave_into_another(gpu):
    """One row of a wave holds NaN, +-inf or 3e38, the other three ordinary numbers: their results are the bits they give when all four rows are ordinary."""
    v, sv, iv, special, out, clean = _row_run()
    assert special.sum() >= 32 and not np.isfinite(out[special][:, :, 1]).all()
    ok = ~special
    same = out[ok].view(np.uint32) == clean[ok].view(np.uint32)
    print(f"{ok.sum()} ordinary rows, {special.sum()} of the waves with a special row: {(~same).sum()} results differ from the all-ordinary launch")
    assert np.isfinite(out[ok][:, :, :5]).all() and same.all()
