"""Test infrastructure: the solver's device building blocks of `judo_amd/csrc/jh_engine_common.h` and `jh_coop.h`, each alone.

`tests/libjudo_amd_xcheck.so` exports `jh_xcheck_blocks` (judo_amd/csrc/jh_xcheck_blocks.hip; no header declares it, it is not product interface).  This module binds it
with ctypes and holds what `tests/test_gpu_solver_blocks.py` (device against reference) and `tests/test_solver_blocks_host.py` (the references against themselves) share:
the input builders -- every number rounded to fp32 FIRST; the device gets the fp32 values, the references the fp64 values of the same numbers -- and the references,
plain numpy statements of each operation.

Every reference takes a `dtype`.  In `np.float64` it is the reference; in `np.float32` it is the reference's own SHADOW: the same statements in the device's number
format.  A tolerance is never taken from the device: each bound is a running-error scale computed from the fp64 reference times a constant, and the constant is 4 times
what the shadow needs on the same cases, rounded up to a power of two (`constant()`).  The factor 4 covers contraction to fma, another order of operations and the 1-ulp
v_rsq / v_rcp.  The constants are written in `C_TOL` next to the measured need; the host test asserts that the shadow still fits a quarter of each.
"""

from __future__ import annotations

import ctypes as C
import glob
import json
import os

import numpy as np

EPS = float(np.finfo(np.float32).eps)  # 2^-23
FAMILY = {"cone": 0, "pyramid": 1, "contact": 2, "impedance": 3, "frame": 4, "chol3": 5, "chol6": 6, "chol7": 7, "chol4": 8, "row": 9, "arm": 10}
IN_F = {"cone": 16, "pyramid": 16, "contact": 16, "impedance": 8, "frame": 4, "chol3": 36, "chol6": 36, "chol7": 36, "chol4": 16, "row": 20, "arm": 64}
OUT_F = {"cone": 24, "pyramid": 24, "contact": 24, "impedance": 1, "frame": 9, "chol3": 44, "chol6": 44, "chol7": 44, "chol4": 24, "row": 28, "arm": 18}
N_CASES = 4096

# The constants of the tolerances: name -> (constant, the shadow's need).  The need is the largest over 8 x 4096 draws of this module's generators (`shadow_needs(0..7)`),
# the constant 4 times that, rounded up to a power of two.  "cone middle f" sits on a power-of-two edge: 4 x 1.9915 = 7.97, so a change of the generators that moves the
# shadow's need past 2.0 turns the constant into 16 and fails the host test here -- that is the rule at work, not a regression.
# FIXED_BOUND names the bounds that are NOT by that rule; the shadow's need stands beside each all the same and the host test holds it under the bound:
#   "frame orthonormal": make_frame's rows are orthonormal to a fixed 8 eps32;
#   "row sums": gsum, qsum4 and row_scatter16 against the fp64 sum, 4 eps32 sum |v| -- four additions deep, half an eps32 of a partial sum each;
#   "chol4 diagonal": |L_pp inv_p - 1| in eps32 -- inv_p is v_rsq(s) to 1 ulp and L_pp = s inv_p, so L_pp inv_p = s inv_p^2 is 1 to 2 * 1 + 1 = 3 eps32; 4 asked.
C_TOL = {
    "cone middle s": (8, 1.26), "cone middle f": (8, 2.00), "cone middle W": (8, 1.61),
    "cone bottom s": (8, 1.49), "cone bottom f": (2, 0.50),
    "cone_dir middle d1": (16, 2.24), "cone_dir middle d2": (16, 3.29), "cone_dir bottom d1": (8, 1.61), "cone_dir bottom d2": (8, 1.50),
    "contact middle s": (8, 1.23), "contact middle f": (16, 2.71), "contact middle W": (8, 1.84),  # (Dm = D0 / (mu^2 (1 + mu^2)) is computed inside contact_eval)
    "pyramid s": (8, 1.19), "pyramid f": (8, 1.31), "pyramid W": (4, 0.98),
    "impedance": (4, 0.64),
    "frame y": (16, 2.31), "frame z": (8, 1.68), "frame parallel": (2, 0.35), "frame cross": (4, 0.63), "frame orthonormal": (8, 3.47),
    "chol factor": (4, 0.70), "chol fwd": (2, 0.45), "chol solve": (4, 0.77),
    "row sums": (4, 1.53), "chol4 diagonal": (4, 1.74),
}
FIXED_BOUND = ("frame orthonormal", "row sums", "chol4 diagonal")


def constant(need: float) -> int:
    """4 x the shadow's need, rounded up to a power of two."""
    return int(2 ** int(np.ceil(np.log2(max(4.0 * need, 1.0)))))


def c_of(name: str) -> int:
    return C_TOL[name][0]


def f32(x) -> np.ndarray:
    """Rounded to fp32, held in fp64."""
    return np.asarray(x, dtype=np.float64).astype(np.float32).astype(np.float64)


# ------------------------------------------------------------------------------------------------ the kernel
_fn = None


def _entry():
    global _fn
    if _fn is None:
        from tests import xcheck

        f = xcheck.load().jh_xcheck_blocks
        f.restype = C.c_int
        f.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
        _fn = f
    return _fn


def launch(family: str, rows: np.ndarray) -> np.ndarray:
    """One launch: `rows` (n, IN_F[family]) fp32 (or its bits) -> (n, OUT_F[family]) fp32.  What the kernel does not write stays NaN."""
    import torch

    from judo_amd import _lib

    rows = np.ascontiguousarray(rows, dtype=np.float32)
    n = rows.shape[0]
    assert rows.shape == (n, IN_F[family]), (family, rows.shape)
    d_in = torch.from_numpy(rows).cuda()
    d_out = torch.full((n, OUT_F[family]), float("nan"), dtype=torch.float32, device="cuda")
    _lib.check(_entry()(FAMILY[family], d_in.data_ptr(), IN_F[family], n, d_out.data_ptr(), OUT_F[family], torch.cuda.current_stream().cuda_stream), "jh_xcheck_blocks")
    torch.cuda.synchronize()
    return d_out.cpu().numpy()


# ------------------------------------------------------------------------------------------------ contact cost: cases
TOP, MIDDLE, BOTTOM = 0, 1, 2
MIN_MARGIN = 1e-4


def cone_NT(c, dtype=np.float64):
    jar, mu, fri = c["jar"].astype(dtype), c["mu"].astype(dtype), c["fri"].astype(dtype)
    return mu * jar[:, 0], fri * np.sqrt(jar[:, 1] ** 2 + jar[:, 2] ** 2)


def cone_zone(c, dtype=np.float64) -> np.ndarray:
    """MuJoCo's zones of the elliptic cone: top (separating, no cost) N >= mu T, bottom (inside the dual cone, quadratic) mu N + T <= 0, middle otherwise."""
    N, T = cone_NT(c, dtype)
    mu = c["mu"].astype(dtype)
    return np.where(N >= mu * T, TOP, np.where(mu * N + T <= 0, BOTTOM, MIDDLE))


def cone_margin(c) -> np.ndarray:
    """How far a case is from the nearer zone boundary, relative: min(|N - mu T|, |mu N + T|) / (|N| + T) in fp64."""
    N, T = cone_NT(c)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.minimum(np.abs(N - c["mu"] * T), np.abs(c["mu"] * N + T)) / (np.abs(N) + T)


def _draw_cone(rng, n, place):
    """`place`: 0 where the draw falls, 1 near the top boundary N = mu T (1 - 10^[-4, -1]), 2 near the bottom boundary N = -(T / mu) (1 +- 10^[-4, -1]).
    The slot's numbers as jh_engine_v5.hip builds them around impedance(csi, dist): D = (D0, D0 impratio, D0 impratio), mu = fri / sqrt(impratio) and
    Dm = D0 / (mu^2 (1 + mu^2)), each evaluated in fp32."""
    F = np.float32
    fri = rng.uniform(0.2, 2.0, n).astype(F)
    impratio = rng.choice([1.0, 3.0, 10.0], n).astype(F)
    D0 = (10.0 ** rng.uniform(1, 5, n)).astype(F)
    D1 = D0 * impratio
    mu = fri / np.sqrt(impratio)
    m2 = mu * mu
    Dm = D0 / (m2 * (F(1) + m2))
    # (one scale for the normal part and one for the tangential pair: the draws that fall where they fall then spread over the three zones)
    jar = f32(rng.standard_normal((n, 3)) * 10.0 ** rng.uniform(-3, 1, (n, 2))[:, [0, 1, 1]])
    jp = f32(rng.standard_normal((n, 3)) * 10.0 ** rng.uniform(-3, 1, (n, 2))[:, [0, 1, 1]])
    mu64, fri64 = mu.astype(np.float64), fri.astype(np.float64)
    T = fri64 * np.sqrt(jar[:, 1] ** 2 + jar[:, 2] ** 2)
    delta = 10.0 ** rng.uniform(-4, -1, n)
    side = rng.choice([-1.0, 1.0], n)
    N = np.where(place == 1, mu64 * T * (1 - delta), -(T / mu64) * (1 + side * delta))
    jar[:, 0] = np.where(place == 0, jar[:, 0], f32(N / mu64))
    return dict(jar=jar, jp=jp, D=np.stack([D0, D1, D1], 1).astype(np.float64), Dm=Dm.astype(np.float64), mu=mu64, fri=fri64,
                d0=f32(rng.standard_normal((n, 2)) * 10.0 ** rng.uniform(-2, 2, (n, 2))), cone=np.ones(n), place=place.astype(np.float64))


def _redraw(rng, n, place, draw, bad_of):
    """Cases drawn until none is `bad`: a bad case is replaced by a fresh draw of the same placement, never dropped (the result has n cases)."""
    c = draw(rng, n, place)
    for _ in range(200):
        bad = np.flatnonzero(bad_of(c))
        if bad.size == 0:
            return c
        new = draw(rng, bad.size, place[bad])
        for k in c:
            c[k][bad] = new[k]
    raise AssertionError("the redraw did not end")


def cone_cases(n: int = N_CASES, seed: int = 0):
    """A third near the top boundary, a sixth near the bottom one, the rest where they fall; a case closer than MIN_MARGIN to a boundary is drawn again."""
    rng = np.random.default_rng(seed)
    place = np.zeros(n, dtype=np.int64)
    place[: n // 3] = 1
    place[n // 3: n // 3 + n // 6] = 2
    return _redraw(rng, n, place, _draw_cone, lambda c: ~(cone_margin(c) >= MIN_MARGIN))


def _case(jar, jp=(0.3, -0.2, 0.1), D0=1024.0, impratio=4.0, fri=1.0, d0=(0.5, -0.25)):
    """One designed case from exact fp32 numbers (fri = 1, impratio = 4: mu = 0.5)."""
    F = np.float32
    mu = F(fri) / np.sqrt(F(impratio))
    m2 = mu * mu
    return dict(jar=f32([jar]), jp=f32([jp]), D=np.array([[D0, D0 * impratio, D0 * impratio]]), Dm=np.array([float(F(D0) / (m2 * (F(1) + m2)))]), mu=np.array([float(mu)]),
                fri=np.array([float(fri)]), d0=f32([d0]), cone=np.ones(1), place=np.zeros(1))


def concat(cs):
    return {k: np.concatenate([c[k] for c in cs]) for k in cs[0]}


EMPTY_SLOT = dict(jar=np.zeros((1, 3)), jp=np.zeros((1, 3)), D=np.zeros((1, 3)), Dm=np.zeros(1), mu=np.zeros(1), fri=np.zeros(1), d0=f32([[0.5, -0.25]]), cone=np.ones(1), place=np.zeros(1))
# name -> case.  T == 0 exactly with N > 0, N < 0 and N == 0 (top, as cone_eval's comment has it); a tangential part whose square underflows to zero / to a denormal in fp32.
DESIGNED_CONE = {
    "T=0 N>0": _case((0.5, 0, 0)), "T=0 N<0": _case((-0.5, 0, 0)), "T=0 N=0": _case((0, 0, 0)),
    "T2 underflows N>0": _case((0.5, 1e-25, 1e-25)), "T2 underflows N<0": _case((-0.5, 1e-25, -1e-25)),
    "T2 denormal N>0": _case((0.5, 1e-20, 0)), "T2 denormal N<0": _case((-0.5, 0, 1e-20)),
    "empty slot": EMPTY_SLOT,
}
# exactly on a zone boundary in fp32 (powers of two throughout: N = mu T, and mu N + T = 0): s, f and d1 are continuous there, W and d2 jump -- either adjacent zone's
DESIGNED_BOUNDARY = {"top boundary": (_case((0.25, 0.25, 0)), (TOP, MIDDLE)), "top boundary, two tangents": (_case((0.625, 0.375, 0.5)), (TOP, MIDDLE)),
                     "bottom boundary": (_case((-1.0, 0, 0.25)), (BOTTOM, MIDDLE)), "bottom boundary, two tangents": (_case((-2.5, 0.375, -0.5)), (BOTTOM, MIDDLE))}


def cone_rows(c) -> np.ndarray:
    n = len(c["mu"])
    r = np.zeros((n, IN_F["cone"]), dtype=np.float32)
    r[:, 0:3], r[:, 3:6], r[:, 6:9], r[:, 9], r[:, 10], r[:, 11], r[:, 12:14], r[:, 14] = c["jar"], c["jp"], c["D"], c["Dm"], c["mu"], c["fri"], c["d0"], c["cone"]
    assert (r.astype(np.float64)[:, :14] == np.concatenate([c["jar"], c["jp"], c["D"], c["Dm"][:, None], c["mu"][:, None], c["fri"][:, None], c["d0"]], 1)).all(), "an input that is no fp32 number"
    return r


def pyramid_rows(c, through_contact_eval: bool) -> np.ndarray:
    """The pyramid's mu (`pmu`) where the family reads it: pyramid_eval's own argument, or contact_eval's `fri`."""
    c = dict(c)
    c["fri" if through_contact_eval else "mu"] = c["pmu"]
    return cone_rows(c)


# ------------------------------------------------------------------------------------------------ contact cost: references
def cone_cost(jar, D, Dm, mu, fri, dtype=np.float64, zone=None):
    """The cost alone, as stated: top 0, bottom 1/2 sum D_i jar_i^2, middle 1/2 Dm (N - mu T)^2 (central differences of THIS tie the derivatives below to it)."""
    jar, D, Dm, mu, fri = (np.asarray(a, dtype) for a in (jar, D, Dm, mu, fri))
    N, T = mu * jar[:, 0], fri * np.sqrt(jar[:, 1] ** 2 + jar[:, 2] ** 2)
    z = np.where(N >= mu * T, TOP, np.where(mu * N + T <= 0, BOTTOM, MIDDLE)) if zone is None else zone
    half = dtype(0.5)
    return np.where(z == TOP, dtype(0), np.where(z == BOTTOM, half * (D * jar * jar).sum(1), half * Dm * (N - mu * T) ** 2)), z


def cone_ref(c, dtype=np.float64, zone=None):
    """Cost s, force f = -ds/djar (n, 3), Hessian W packed 00, 10, 11, 20, 21, 22 (n, 6), cone_dir's d1 = d1_0 - f . jp and d2 = d2_0 + jp' W jp (written along the
    line: s' = Dm e e', s'' = Dm (e'^2 + e e'') with e = N - mu T), the zone, and the running-error scales of each (fp64 only; a scale of 0 asks for the exact value)."""
    jar, jp, D, Dm, mu, fri, d0 = (c[k].astype(dtype) for k in ("jar", "jp", "D", "Dm", "mu", "fri", "d0"))
    n = len(mu)
    s, z = cone_cost(jar, D, Dm, mu, fri, dtype, zone)
    N, T = mu * jar[:, 0], fri * np.sqrt(jar[:, 1] ** 2 + jar[:, 2] ** 2)
    e = N - mu * T
    with np.errstate(all="ignore"):
        iT = np.where(T > 0, dtype(1) / np.where(T > 0, T, dtype(1)), dtype(0))
        # middle: ds/dj0 = Dm e mu, ds/djk = -Dm e mu fri^2 jk / T;  H00 = Dm mu^2, H0k = -Dm mu^2 fri^2 jk / T, Hkl = Dm mu^2 tk tl - Dm e mu (fri^2 dkl - tk tl) / T, tk = fri^2 jk / T
        t1, t2 = fri * fri * jar[:, 1] * iT, fri * fri * jar[:, 2] * iT
        gm = np.stack([Dm * e * mu, -Dm * e * mu * t1, -Dm * e * mu * t2], 1)
        k1, k2 = Dm * mu * mu, Dm * e * mu * iT
        Wm = np.stack([k1, -k1 * t1, k1 * t1 * t1 - k2 * (fri * fri - t1 * t1), -k1 * t2, (k1 + k2) * t1 * t2, k1 * t2 * t2 - k2 * (fri * fri - t2 * t2)], 1)
        V0, V1, V2 = mu * jp[:, 0], fri * jp[:, 1], fri * jp[:, 2]
        Tp = (fri * jar[:, 1] * V1 + fri * jar[:, 2] * V2) * iT
        Tpp = (V1 * V1 + V2 * V2 - Tp * Tp) * iT
        ep = V0 - mu * Tp
        d1m, d2m = Dm * e * ep, Dm * (ep * ep - e * mu * Tpp)
    zero = np.zeros(n, dtype)
    gb = D * jar
    Wb = np.stack([D[:, 0], zero, D[:, 1], zero, zero, D[:, 2]], 1)
    d1b, d2b = (D * jar * jp).sum(1), (D * jp * jp).sum(1)
    zc = z[:, None]
    f = -np.where(zc == TOP, dtype(0), np.where(zc == BOTTOM, gb, gm))
    W = np.where(zc == TOP, dtype(0), np.where(zc == BOTTOM, Wb, Wm))
    d1 = d0[:, 0] + np.where(z == TOP, dtype(0), np.where(z == BOTTOM, d1b, d1m))
    d2 = d0[:, 1] + np.where(z == TOP, dtype(0), np.where(z == BOTTOM, d2b, d2m))
    out = dict(s=s, f=f, W=W, d1=d1, d2=d2, zone=z)
    if dtype is np.float64:
        # The middle zone carries the cancellation in e = N - mu T: with A = |N| + mu T the cost has eps (Dm |e| A + s), the force eps Dm mu A max(1, fri), the Hessian
        # eps Dm max(mu, fri)^2 (1 + mu A / T).  Along jp, e' = V0 - mu T' has the error eps Ap, Ap = |V0| + mu |Vt|, and T'' = (|Vt|^2 - T'^2) / T is at most |Vt|^2 / T:
        # d1 eps Dm A Ap, d2 eps Dm (Ap^2 + A mu |Vt|^2 / T).  Top and bottom have no cancellation: eps sum |terms|.  cone_dir adds the value it was given: + eps |d_0|.
        A = np.abs(N) + mu * T
        Vt = np.sqrt(V1 * V1 + V2 * V2)
        Ap = np.abs(V0) + mu * Vt
        mf = np.maximum(mu, fri)
        with np.errstate(all="ignore"):
            sm = dict(s=Dm * np.abs(e) * A + s, f=Dm * mu * A * np.maximum(1.0, fri), W=Dm * mf * mf * (1 + mu * A * iT), d1=Dm * A * Ap, d2=Dm * (Ap * Ap + A * mu * Vt * Vt * iT))
        sb = dict(s=0.5 * (D * jar * jar).sum(1), f=np.abs(D * jar), W=zero, d1=np.abs(D * jar * jp).sum(1), d2=(D * jp * jp).sum(1))
        sc = {}
        for k in ("s", "f", "W", "d1", "d2"):
            m, b = (sm[k][:, None], sb[k] if sb[k].ndim == 2 else sb[k][:, None]) if k in ("f", "W") else (sm[k], sb[k])
            zz = zc if k in ("f", "W") else z
            sc[k] = EPS * np.where(zz == TOP, 0.0, np.where(zz == BOTTOM, b, m))
        sc["f"], sc["W"] = np.broadcast_to(sc["f"], (n, 3)).copy(), np.broadcast_to(sc["W"], (n, 6)).copy()
        sc["d1"] = sc["d1"] + EPS * np.abs(d0[:, 0]) * (z != TOP)
        sc["d2"] = sc["d2"] + EPS * np.abs(d0[:, 1]) * (z != TOP)
        out["scale"] = sc
    return out


def need(got, ref, scale, mask=None) -> float:
    """The largest |got - ref| / scale; where the scale is 0 the value must be the reference's exactly (inf otherwise)."""
    got, ref, scale = np.broadcast_arrays(np.asarray(got, np.float64), np.asarray(ref, np.float64), np.asarray(scale, np.float64))
    if mask is not None:
        m = np.broadcast_to(mask.reshape(mask.shape + (1,) * (got.ndim - mask.ndim)), got.shape)
        got, ref, scale = got[m], ref[m], scale[m]
    if got.size == 0:
        return 0.0
    err = np.abs(got - ref)
    with np.errstate(all="ignore"):
        r = np.where(scale > 0, err / np.where(scale > 0, scale, 1.0), np.where(err == 0, 0.0, np.inf))
    r = np.where(np.isnan(r), np.inf, r)
    return float(r.max())


# ---- pyramid
def pyramid_margin(c) -> np.ndarray:
    """Relative distance of the nearest of the four rows jar_n +- mu jar_t from 0 (its sign decides whether the row is active)."""
    j, mu = c["jar"], c["pmu"]
    m = np.full(len(mu), np.inf)
    for k in range(4):
        sg = -mu if k & 1 else mu
        t = j[:, 1] if k < 2 else j[:, 2]
        with np.errstate(all="ignore"):
            m = np.minimum(m, np.abs(j[:, 0] + sg * t) / (np.abs(j[:, 0]) + mu * np.abs(t)))
    return m


def _draw_pyramid(rng, n, place):
    c = _draw_cone(rng, n, np.zeros(n, dtype=np.int64))
    # the tangential parts on the normal's own scale for half of the draws: all four rows active, or none, then depends on a sign alone and not on a ratio of scales
    same = rng.random(n) < 0.5
    c["jar"][:, 1:] = np.where(same[:, None], f32(c["jar"][:, :1] * rng.uniform(-0.6, 0.6, (n, 2))), c["jar"][:, 1:])
    c["pmu"] = np.where(place == 1, c["fri"], c["mu"])  # what pyramid_eval gets as mu: the tree kernels' slot mu (family "pyramid"), contact_eval's `fri` (family "contact")
    c["cone"] = np.zeros(n)
    return c


def pyramid_cases(n: int = N_CASES, seed: int = 1, through_contact_eval: bool = False):
    rng = np.random.default_rng(seed)
    return _redraw(rng, n, np.full(n, int(through_contact_eval)), _draw_pyramid, lambda c: ~(pyramid_margin(c) >= MIN_MARGIN))


def pyramid_cost(jar, D0, mu, dtype=np.float64, rows=(0, 1, 2, 3)):
    """1/2 D sum of min(0, jar_n +- mu jar_t1, jar_n +- mu jar_t2)^2: four one-sided rows (`rows`: some of them alone -- the cost is their sum)."""
    jar, D0, mu = (np.asarray(a, dtype) for a in (jar, D0, mu))
    s = np.zeros(len(mu), dtype)
    for k in rows:
        x = jar[:, 0] + (-mu if k & 1 else mu) * (jar[:, 1] if k < 2 else jar[:, 2])
        s = s + dtype(0.5) * D0 * np.minimum(x, dtype(0)) ** 2
    return s


def pyramid_ref(c, dtype=np.float64):
    """s, f = -ds/djar, W = sum over the active rows of D r r' with r = (1, +-mu, 0) / (1, 0, +-mu); a row at exactly 0 is inactive.  `nact`: the number of active rows."""
    jar, D0, mu = c["jar"].astype(dtype), c["D"][:, 0].astype(dtype), c["pmu"].astype(dtype)
    n = len(mu)
    s, g, H, nact = np.zeros(n, dtype), np.zeros((n, 3), dtype), np.zeros((n, 3, 3), dtype), np.zeros(n, dtype=np.int64)
    X2, X1 = np.zeros(n), np.zeros(n)
    for k in range(4):
        sg = -mu if k & 1 else mu
        t = 1 if k < 2 else 2
        r = np.zeros((n, 3), dtype); r[:, 0] = 1; r[:, t] = sg
        x = jar[:, 0] + sg * jar[:, t]
        act = x < 0
        xa = np.where(act, x, dtype(0))
        s = s + dtype(0.5) * D0 * xa * xa
        g = g + (D0 * xa)[:, None] * r
        H = H + np.where(act, D0, dtype(0))[:, None, None] * r[:, :, None] * r[:, None, :]
        nact += act
        X = np.abs(jar[:, 0]).astype(np.float64) + np.abs(sg * jar[:, t]).astype(np.float64)
        X2, X1 = X2 + act * X * X, X1 + act * X
    out = dict(s=s, f=-g, W=np.stack([H[:, 0, 0], H[:, 1, 0], H[:, 1, 1], H[:, 2, 0], H[:, 2, 1], H[:, 2, 2]], 1), nact=nact)
    if dtype is np.float64:
        # a row x = jar_n +- mu jar_t has the error eps X, X = |jar_n| + mu |jar_t|: the cost eps D sum X^2, the force eps D max(1, mu) sum X, the weights eps max(1, mu)^2 D n_active
        m1 = np.maximum(1.0, mu)
        out["scale"] = dict(s=EPS * D0 * X2, f=np.broadcast_to((EPS * D0 * m1 * X1)[:, None], (n, 3)).copy(), W=np.broadcast_to((EPS * D0 * m1 * m1 * nact)[:, None], (n, 6)).copy())
    return out


def _pcase(jar, mu=0.5, D0=1024.0):
    c = _case(jar)
    c["pmu"], c["cone"], c["D"] = np.array([mu]), np.zeros(1), np.array([[D0, D0, D0]])
    return c


# all four rows active, none, one row at exactly 0 (j0 = mu j1: inactive) with its opposite row active, everything 0
DESIGNED_PYRAMID = {"four rows": _pcase((-1.0, 0.5, -0.25)), "no row": _pcase((1.0, 0.5, -0.25)), "a row at 0": _pcase((-0.25, 0.5, 0.125)), "a row at 0, none active": _pcase((0.25, 0.5, 0.0)),
                    "all zero": _pcase((0.0, 0.0, 0.0))}


def contact_ref(c, dtype=np.float64):
    """contact_eval: cone == 1 is cone_eval with Dm = D0 / (mu^2 (1 + mu^2)) computed there, anything else pyramid_eval(jar, D[0], fri)."""
    c = dict(c)
    mu, D0 = c["mu"].astype(dtype), c["D"][:, 0].astype(dtype)
    c["Dm"] = D0 / (mu * mu * (dtype(1) + mu * mu))
    return cone_ref(c, dtype)


# ------------------------------------------------------------------------------------------------ impedance
def impedance(si, dist, dtype=np.float64):
    """MuJoCo's impedance d(x) of solimp = (d0, d1, width, midpoint, power) at x = |dist| / width, as the oracle states it (elementwise; scalars give a scalar).
    The mean of d0 and d1 where they are equal or the width is at most 1e-15 (mjMINVAL, here the fp32 number the device compares with)."""
    d0, d1, width, mid, power = (np.asarray(a, dtype) for a in si)
    dist = np.asarray(dist, dtype)
    one = dtype(1)
    with np.errstate(all="ignore"):
        x = np.minimum(np.abs(dist) / width, one)
        y = np.where(power == 1, x, np.where(x <= mid, x**power / mid ** (power - one), one - (one - x) ** power / (one - mid) ** (power - one)))
        out = np.where((d0 == d1) | (width <= dtype(np.float32(1e-15))), dtype(0.5) * (d0 + d1), d0 + y * (d1 - d0))
    return out if out.ndim else out[()]


def model_solimps() -> list[tuple]:
    """Every distinct solimp of judo_amd/models/*.json (any key that starts with `solimp`)."""
    found = set()

    def walk(o):
        if isinstance(o, dict):
            for k, v in o.items():
                if k.startswith("solimp") and isinstance(v, list) and len(v) == 5 and all(isinstance(x, (int, float)) for x in v):
                    found.add(tuple(float(x) for x in v))
                else:
                    walk(v)
        elif isinstance(o, list):
            for v in o:
                walk(v)

    root = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "judo_amd", "models")
    for p in sorted(glob.glob(os.path.join(root, "*.json"))):
        walk(json.load(open(p)))
    return sorted(found)


def impedance_cases():
    """(si (n, 5), dist (n), group (n)): per solimp a dense sweep over [-1.5, 1.5] widths, 0, +-width and `midpoint * width` (evaluated in fp32) with their fp32 neighbours;
    every dist comes with -dist.  All through judo_amd.models.clamp_solimp, as every caller's."""
    from judo_amd.models import clamp_solimp

    base = (0.9, 0.95, 0.001)
    sis = list(model_solimps())
    sis += [base + (mid, p) for mid in (1e-4, 0.5, 0.9999) for p in (1.0, 2.0, 1.5, 3.0, 6.0)]
    sis += [(0.95, 0.3, 0.01, 0.5, 2.0), (0.95, 0.3, 0.01, 0.25, 3.0), (0.9, 0.9, 0.001, 0.5, 2.0), (0.9, 0.95, 1e-15, 0.5, 2.0), (0.9, 0.95, 2e-15, 0.5, 2.0), (0.9, 0.95, 2e-15, 0.3, 1.5),
            (0.0, 1.0, 0.001, 0.5, 2.0), (0.5, 2.0, -1.0, 2.0, 0.5)]  # (the last two are clamped: d0, d1 and the midpoint into [1e-4, 0.9999], the width to 0, the power to 1)
    F = np.float32
    S, Dd, G = [], [], []
    for g, si in enumerate(sis):
        si32 = np.asarray(clamp_solimp(list(si)), dtype=F)
        w = si32[2] if si32[2] > 0 else F(1e-3)
        d = [np.linspace(-1.5, 1.5, 193).astype(F) * w]
        for v in (F(0), w, si32[3] * w):
            d.append(np.array([v, np.nextafter(v, F(np.inf)), np.nextafter(v, F(-np.inf))], dtype=F))
        d = np.concatenate(d)
        d = np.unique(np.concatenate([d, -d]))
        S.append(np.broadcast_to(si32, (d.size, 5))); Dd.append(d); G.append(np.full(d.size, g))
    return np.concatenate(S).astype(np.float64), np.concatenate(Dd).astype(np.float64), np.concatenate(G)


# ------------------------------------------------------------------------------------------------ make_frame
def frame_ref(nrm, dtype=np.float64, use_z=None):
    """MuJoCo's mju_makeFrame as the oracle states it: x the normalised input, y the y axis -- the z axis where |x_y| > 0.5 -- made orthogonal to x and normalised, z = x cross y.
    `use_z` forces the choice of the axis."""
    v = np.asarray(nrm, dtype)
    x = v / np.sqrt((v * v).sum(1))[:, None]
    if use_z is None:
        use_z = (x[:, 1] < dtype(-0.5)) | (x[:, 1] > dtype(0.5))
    e = np.where(use_z[:, None], np.array([0, 0, 1], dtype), np.array([0, 1, 0], dtype))
    y = e - x * (x * e).sum(1)[:, None]
    with np.errstate(all="ignore"):
        y = y / np.sqrt((y * y).sum(1))[:, None]
    return x, y, np.cross(x, y).astype(dtype), use_z


def frame_cases(n: int = N_CASES, seed: int = 2):
    """Random directions of length 0.1 to 10, the six axes, and normals whose normalised y component is +-0.5, with the fp32 neighbours of that."""
    rng = np.random.default_rng(seed)
    v = rng.standard_normal((n, 3))
    v *= (rng.uniform(0.1, 10, n) / np.linalg.norm(v, axis=1))[:, None]
    ax = np.concatenate([np.eye(3), -np.eye(3)]) * np.array([1, 0.1, 10, 3, 0.5, 7])[:, None]
    th = rng.uniform(0, 2 * np.pi, 64)
    edge = np.stack([np.sqrt(0.75) * np.cos(th), np.where(np.arange(64) % 2, -0.5, 0.5), np.sqrt(0.75) * np.sin(th)], 1) * np.repeat([1.0, 0.1, 10.0, 2.0], 16)[:, None]
    edge = edge.astype(np.float32)
    nb = []
    for k in (-64, -2, -1, 0, 1, 2, 64):  # (one fp32 step of the y component is an eighth to a quarter of an eps32 of |x_y|)
        e = edge.copy()
        for _ in range(abs(k)):
            e[:, 1] = np.nextafter(e[:, 1], np.float32(np.inf if k > 0 else -np.inf))
        nb.append(e)
    return np.concatenate([f32(v), f32(ax)] + [b.astype(np.float64) for b in nb])


# ------------------------------------------------------------------------------------------------ packed Cholesky
def tri_index(N):
    return [(p, m) for p in range(N) for m in range(p + 1)]


def pack(A):
    N = A.shape[-1]
    return np.stack([A[:, p, m] for p, m in tri_index(N)], 1)


def unpack(a, N):
    """Packed lower triangle (n, N (N + 1) / 2) -> lower-triangular (n, N, N)."""
    L = np.zeros((a.shape[0], N, N), dtype=a.dtype)
    for k, (p, m) in enumerate(tri_index(N)):
        L[:, p, m] = a[:, k]
    return L


def spd_cases(N: int, n: int = N_CASES, seed: int = 3):
    """(A (n, N, N) symmetric, fp32 numbers; b (n, N); kind (n): 0 Q diag(lambda) Q' with condition number 10^[0, 4] and scale 10^[-3, 3], 1 the same block-diagonal,
    2 a pivot at or below zero -- the last four cases, see below)."""
    rng = np.random.default_rng(seed + 100 * N)
    A, kind = np.zeros((n, N, N)), np.zeros(n, dtype=np.int64)

    def spd(m, cond, scale):
        Q, _ = np.linalg.qr(rng.standard_normal((m, m)))
        lam = scale * cond ** (-np.linspace(0, 1, m) if m > 1 else np.zeros(1))
        return (Q * lam) @ Q.T

    for i in range(n):
        cond, scale = 10.0 ** rng.uniform(0, 4), 10.0 ** rng.uniform(-3, 3)
        if i % 4 == 3:
            h = N // 2
            A[i, :h, :h], A[i, h:, h:], kind[i] = spd(h, cond, scale), spd(N - h, 10.0 ** rng.uniform(0, 4), scale * 10.0 ** rng.uniform(-1, 1)), 1
        else:
            A[i] = spd(N, cond, scale)
    # The cases that reach the pivot clamp fmaxf(d, 1e-30f), the last four (kind 2).  Three have a pivot that is EXACT in fp32 whatever the contraction and the order:
    # row and column p all zero (every term of the pivot is 0 * x: the pivot is 0), a diagonal entry of -1 in such a row (the pivot is -1), and a leading block
    # [[4, 4], [4, 4]] (the second pivot is 4 - 2 * 2 = 0 where v_rsq(4) is exactly 0.5, and rounding noise of either sign where it is not).  The fourth is B B' with small
    # integers, of rank N - 1: its last pivot is rounding noise.  CLAMPED_PIVOT says which pivot of which case must come out as rsq(1e-30).
    p = N // 2
    for k in (4, 3):
        A[n - k, p, :] = 0
        A[n - k, :, p] = 0
    A[n - 3, p, p] = -1.0
    A[n - 2] = np.eye(N) * 4.0
    A[n - 2, 1, 0] = A[n - 2, 0, 1] = 4.0
    B = rng.integers(-3, 4, (N, N - 1)).astype(np.float64)
    A[n - 1] = B @ B.T
    kind[n - 4:] = 2
    A = unpack(f32(pack(A)), N)
    A = A + np.transpose(np.tril(A, -1), (0, 2, 1))
    b = f32(rng.standard_normal((n, N)) * 10.0 ** rng.uniform(-2, 2, (n, 1)))
    return A, b, kind


def clamped_pivots(N: int, n: int) -> dict:
    """case index -> the pivot of spd_cases(N, n) that is exactly 0 or -1 in fp32 and must be clamped."""
    return {n - 4: N // 2, n - 3: N // 2}


RSQ_CLAMP = 1.0 / np.sqrt(np.float64(np.float32(1e-30)))  # what a clamped pivot's reciprocal root is: v_rsq_f32(1e-30f), good to 1 ulp, i.e. to eps32 of this


def chol_shadow(A, b, dtype=np.float32, pivots=False):
    """chol_packed / fwd_packed / bwd_packed restated in numpy: (L lower with its true diagonal, y = L^-1 b, x = L^-T y); with `pivots`, also the pivots before the clamp
    and their reciprocal roots."""
    A, b = A.astype(dtype), b.astype(dtype)
    n, N = b.shape
    L, inv = np.zeros_like(A), np.zeros((n, N), dtype)
    piv = np.zeros((n, N), dtype)
    with np.errstate(all="ignore"):  # (the singular cases overflow)
        out = _chol_shadow(A, b, L, inv, piv, dtype)
    return out + (piv, inv) if pivots else out


def _chol_shadow(A, b, L, inv, piv, dtype):
    n, N = b.shape
    for p in range(N):
        for m in range(p):
            s = A[:, p, m].copy()
            for q in range(m):
                s = s - L[:, p, q] * L[:, m, q]
            L[:, p, m] = s * inv[:, m]
        d = A[:, p, p].copy()
        for q in range(p):
            d = d - L[:, p, q] * L[:, p, q]
        piv[:, p] = d
        inv[:, p] = dtype(1) / np.sqrt(np.maximum(d, dtype(1e-30)))
        L[:, p, p] = dtype(1) / inv[:, p]
    y = np.zeros((n, N), dtype)
    for m in range(N):
        s = b[:, m].copy()
        for q in range(m):
            s = s - y[:, q] * L[:, m, q]
        y[:, m] = s * inv[:, m]
    x = np.zeros((n, N), dtype)
    for m in range(N - 1, -1, -1):
        s = y[:, m].copy()
        for q in range(m + 1, N):
            s = s - L[:, q, m] * x[:, q]
        x[:, m] = s * inv[:, m]
    return L, y, x


def chol_needs(A, b, L, y, x):
    """Residuals in fp64 over their scales, per case: factor ||L L' - A||_max / (N eps ||A||_max), forward solve ||L y - b||_inf / (N eps ||L||_inf ||y||_inf), the whole
    solve ||A x - b||_inf / (N eps ||A||_inf ||x||_inf).  Residuals, not forward errors: they do not grow with the condition number."""
    A, b, L, y, x = (np.asarray(a, np.float64) for a in (A, b, L, y, x))
    N = b.shape[1]
    inf_norm = lambda M: np.abs(M).sum(2).max(1)  # noqa: E731
    fac = np.abs(L @ np.transpose(L, (0, 2, 1)) - A).max((1, 2)) / (N * EPS * np.abs(A).max((1, 2)))
    fwd = np.abs(np.einsum("nij,nj->ni", L, y) - b).max(1) / (N * EPS * inf_norm(L) * np.abs(y).max(1))
    sol = np.abs(np.einsum("nij,nj->ni", A, x) - b).max(1) / (N * EPS * inf_norm(A) * np.abs(x).max(1))
    return fac, fwd, sol


# ------------------------------------------------------------------------------------------------ row reductions: fp32 emulation of the documented pairing orders
LANE = np.arange(16)
XOR1, XOR2, HALF_MIRROR, MIRROR = LANE ^ 1, LANE ^ 2, np.where(LANE < 8, 7 - LANE, 23 - LANE), 15 - LANE
ROR4, ROR8 = (LANE - 4) % 16, (LANE - 8) % 16  # row_ror:n -- lane i reads lane i - n of its row


def _step(v, perm):
    with np.errstate(all="ignore"):
        return v + v[:, perm]


def emu_csum(v):
    """(rows, 16) fp32 -> the same shape: xor 1, xor 2."""
    return _step(_step(v.astype(np.float32), XOR1), XOR2)


def emu_gsum(v):
    return _step(_step(emu_csum(v), HALF_MIRROR), MIRROR)


def emu_qsum4(v):
    return _step(_step(v.astype(np.float32), ROR4), ROR8)


def emu_qsum4_same(v):
    return _step(_step(v.astype(np.float32), ROR8), ROR4)


def emu_row_scatter16(V):
    """(rows, 16 lanes, 16 values) fp32 -> (rows, 16): the four select-and-add levels -- mirror, half mirror, xor 2, xor 1; lane l keeps the half of its values whose
    index shares its next lane bit and adds its partner's copy of that half."""
    k = V.astype(np.float32)
    for bit, perm in ((8, MIRROR), (4, HALF_MIRROR), (2, XOR2), (1, XOR1)):
        h = k.shape[2] // 2
        up = ((LANE & bit) != 0)[None, :, None]
        keep, send = np.where(up, k[:, :, h:], k[:, :, :h]), np.where(up, k[:, :, :h], k[:, :, h:])
        with np.errstate(all="ignore"):
            k = keep + send[:, perm, :]
    return k[:, :, 0]


def same_bits(a, b) -> np.ndarray:
    """Elementwise: the same fp32 bits, or both NaN (a NaN's payload is nobody's claim)."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


def row_cases(seed: int = 4):
    """Rows of 16 lanes: v (R, 16) fp32, sv (R, 16, 16) fp32, iv (R, 16) int32, and `special` (R): the row holds NaN, +-inf or 3e38.  R is a multiple of 4 (four rows are a
    wave) and every special row sits among three ordinary ones."""
    rng = np.random.default_rng(seed)
    F = np.float32
    R = 1024

    def mixed(shape):
        return (rng.standard_normal(shape) * 10.0 ** rng.uniform(-6, 6, shape)).astype(F)

    v, sv = mixed((R, 16)), mixed((R, 16, 16))
    iv = rng.integers(-2**31, 2**31, (R, 16), dtype=np.int64).astype(np.int32)
    # exact cancellations: pairs x, -x across every pairing distance, and a large pair around a small sum
    for r in range(0, 64):
        x = mixed(16)
        d = (1, 2, 4, 8)[r % 4]
        v[r] = np.where((LANE & d) != 0, -x[LANE ^ d], x)
    for r in range(64, 96):
        v[r] = mixed(16) * F(1e-6); v[r, r % 16] = F(3e6); v[r, (r * 7 + 3) % 16 if (r * 7 + 3) % 16 != r % 16 else (r + 1) % 16] = F(-3e6)
    # denormals, alone and among normal numbers; small ints, negative ints, INT_MIN
    v[96:128] = (rng.standard_normal((32, 16)) * 10.0 ** rng.uniform(-45, -38, (32, 16))).astype(F)
    v[128:160, ::3] = (rng.standard_normal((32, 6)) * 1e-41).astype(F)
    sv[96:128] = (rng.standard_normal((32, 16, 16)) * 10.0 ** rng.uniform(-45, -38, (32, 16, 16))).astype(F)
    iv[0:64] = rng.integers(-5, 6, (64, 16)); iv[64:96] = rng.integers(-1000, 0, (32, 16)); iv[96:128, 5] = -2**31; iv[128:160] = 1 << rng.integers(0, 32, (32, 16)).astype(np.int64) - 0
    iv[160:192] = 0; iv[160:192, 9] = -2**31  # the sign bit alone, in one lane
    special = np.zeros(R, dtype=bool)
    bad = [F(np.nan), F(np.inf), F(-np.inf), F(3e38), F(-3e38)]
    for w, r in enumerate(range(256, 512, 4)):  # one row of each of these waves
        rr = r + w % 4
        special[rr] = True
        b = bad[w % 5]
        lanes = rng.choice(16, 1 + w % 3, replace=False)
        v[rr, lanes] = b
        sv[rr, lanes, :] = b
        if w % 7 == 0:
            v[rr, :] = b  # (the whole row: an all-NaN row is gmin's only NaN)
    return v, sv, iv, special


def row_rows(v, sv, iv) -> np.ndarray:
    R = v.shape[0]
    r = np.zeros((R * 16, IN_F["row"]), dtype=np.float32)
    r[:, 0], r[:, 1:17], r[:, 17] = v.reshape(-1), sv.reshape(-1, 16), iv.reshape(-1).view(np.float32)
    return r


# ------------------------------------------------------------------------------------------------ the arm's 9 x 9 system
def arm_rows(A, b) -> np.ndarray:
    """Per DPP row one system: lane 6 + a gets row a of A in its entries b <= a -- the entries it owns -- and unrelated numbers above the diagonal, lane 15 the right-hand
    side, lanes 0-5 (the free body's, whose values the routine never reads into x) unrelated numbers throughout; every lane also gets the whole system for chol_solve<9>."""
    n = A.shape[0]
    rng = np.random.default_rng(5)
    r = np.zeros((n, 16, IN_F["arm"]), dtype=np.float32)
    junk = f32(rng.standard_normal((n, 16, 9)) * np.abs(A).max((1, 2))[:, None, None])
    for l in range(16):
        row = junk[:, l].copy()
        if l == 15:
            row = b
        elif l >= 6:
            row[:, : l - 5] = A[:, l - 6, : l - 5]
        r[:, l, 0:9] = row
    r[:, :, 9:54], r[:, :, 54:63] = pack(A)[:, None, :], b[:, None, :]
    return r.reshape(n * 16, IN_F["arm"])


# ------------------------------------------------------------------------------------------------ what the shadow needs
def frame_ambiguous(nrm) -> np.ndarray:
    """The fp64 normalised |x_y| lies within 4 eps32 of 0.5: either tangent is right."""
    x = np.asarray(nrm, np.float64)
    return np.abs(np.abs(x[:, 1]) / np.sqrt((x * x).sum(1)) - 0.5) <= 4 * EPS


def frame_needs(nrm, x, y, z):
    """A frame (x, y, z) for the normals `nrm` against the fp64 reference, in units of eps32: (y, z, x parallel to the input, z = x cross y, rows orthonormal); y and z
    over the cases whose tangent choice is the reference's, with `chosen_ok` saying where it is (or may be either)."""
    x, y, z = (np.asarray(a, np.float64) for a in (x, y, z))
    rx, ry, rz, use_z = frame_ref(nrm)
    other = frame_ref(nrm, use_z=~use_z)[1]
    with np.errstate(all="ignore"):
        chosen = ~(np.abs(y - other).max(1) < np.abs(y - ry).max(1))  # (the tangent built from the reference's axis is the nearer of the two candidates)
    ok = chosen | frame_ambiguous(nrm)
    ny = np.where(chosen, np.abs(y - ry).max(1), 0.0) / EPS
    nz = np.where(chosen, np.abs(z - rz).max(1), 0.0) / EPS
    par = np.abs(np.cross(x, nrm)).max(1) / np.linalg.norm(nrm, axis=1) / EPS + np.where((x * nrm).sum(1) > 0, 0.0, np.inf)
    crs = np.abs(z - np.cross(x, y)).max(1) / EPS
    Rm = np.stack([x, y, z], 1)
    orth = np.abs(Rm @ np.transpose(Rm, (0, 2, 1)) - np.eye(3)).max((1, 2)) / EPS
    return dict(y=ny, z=nz, parallel=par, cross=crs, orthonormal=orth, chosen_ok=ok)


def shadow_needs(seed: int = 0) -> dict:
    """name of C_TOL -> what the fp32 shadow of the reference needs of that scale on this module's cases (the host test holds each to a quarter of its constant, a
    FIXED_BOUND to the bound).  `seed` 0: the cases the tests run; another seed: further draws of the same generators."""
    F, out = np.float32, {}
    for fam, ref_of in (("cone", cone_ref), ("contact", contact_ref)):
        c = cone_cases(seed=1000 * seed)
        r, s = ref_of(c), ref_of(c, F)
        assert (r["zone"] == s["zone"]).all()
        for zname, z in (("middle", MIDDLE), ("bottom", BOTTOM)):
            for k in ("s", "f", "W") + (("d1", "d2") if fam == "cone" else ()):
                name = f"{'cone_dir' if k in ('d1', 'd2') else 'cone' if zname == 'bottom' else fam} {zname} {k}"
                if name in C_TOL:
                    out[name] = max(out.get(name, 0.0), need(s[k], r[k], r["scale"][k], r["zone"] == z))
    for through in (False, True):
        c = pyramid_cases(seed=1000 * seed + 1, through_contact_eval=through)
        r, s = pyramid_ref(c), pyramid_ref(c, F)
        assert (r["nact"] == s["nact"]).all()
        for k in ("s", "f", "W"):
            out[f"pyramid {k}"] = max(out.get(f"pyramid {k}", 0.0), need(s[k], r[k], r["scale"][k]))
    si, dist, _ = impedance_cases()
    out["impedance"] = float(np.abs(impedance(si.T, dist, F).astype(np.float64) - impedance(si.T, dist)).max() / EPS)
    nrm = frame_cases(seed=1000 * seed + 2)
    fn = frame_needs(nrm, *frame_ref(nrm, F)[:3])
    assert fn["chosen_ok"].all()
    for k in ("y", "z", "parallel", "cross", "orthonormal"):
        out[f"frame {k}"] = float(fn[k].max())
    for N in (3, 4, 6, 7, 9):
        A, b, kind = spd_cases(N, seed=1000 * seed + 3)
        L, y, x, piv, inv = chol_shadow(A, b, pivots=True)
        fac, fwd, sol = chol_needs(A, b, L, y, x)
        for k, v in (("factor", fac), ("fwd", fwd), ("solve", sol)):
            out[f"chol {k}"] = max(out.get(f"chol {k}", 0.0), float(v[kind != 2].max()))
        if N == 4:  # chol4 keeps L_pp = s * inv_p beside inv_p = 1 / sqrt(s)
            ok = kind != 2
            out["chol4 diagonal"] = float(np.abs((piv[ok] * inv[ok]).astype(np.float64) * inv[ok] - 1).max() / EPS)
    v, sv, _, special = row_cases(seed=1000 * seed + 4)
    ok = ~special
    x, X = v[ok].astype(np.float64), sv[ok].astype(np.float64)
    q = lambda a: a.reshape(-1, 4, 4)  # noqa: E731  [row, quad, position in the quad]: qsum4 sums over the quads
    out["row sums"] = float(max((np.abs(emu_gsum(v[ok]) - x.sum(1, keepdims=True)) / (EPS * np.abs(x).sum(1, keepdims=True))).max(),
                                (np.abs(q(emu_qsum4(v[ok]).astype(np.float64)) - q(x).sum(1, keepdims=True)) / (EPS * np.abs(q(x)).sum(1, keepdims=True))).max(),
                                (np.abs(emu_row_scatter16(sv[ok]) - X.sum(1)) / (EPS * np.abs(X).sum(1))).max()))
    return out
