// jh_image.h -- the packed image of an articulated model (judo_amd/engine_model.py::pack_engine_model writes it): the one definition of its layout, the view every
// kernel and the host take of it, and the host's readers.  No HIP in here: a plain C++ compiler reads it too (tests/image_view_check.cpp).
//
// The image is a float section F and an int section I behind the 64-byte blob header.  In file order (a record size in brackets; `*`: leap family only, `+`: caltech only):
//
//   I  header [HEADER_I]: the HI_* slots below                         F  header [HEADER_F]: HF_*
//      bodies NM x [BODY_I]: parent, joint type, dof, qpos, block, depth    bodies NM x [BODY_F]: BF_*
//      blocks NBLK x [BLOCK_I]                                              dofs NV x [DOF_F]: DF_*
//      actuators NU x [ACT_I]: dof, qpos                                    actuators NU x [ACT_F]: AF_*
//      geoms NG x [GEOM_I]: body, type                                      geoms NG x [GEOM_F]: GF_*
//      sites NSITE x [1]: body                                              sites NSITE x [SITE_F]
//      sensors NSENS x [SENS_I]: type, object, address
//    * lane lists at I[HI_LANES]: LANES x I[HI_LGM] geoms
//    * body pairs at I[HI_BP]: I[HI_NBP] x [2], then                      * bounding volumes at I[HI_BS]: BODY_CODES x [BV_F]
//      BODY_CODES x [2]: first geom, count
//      generic block at I[HI_GI]: [GEN_I] counts (GI_*), then               generic block at I[HI_GF]:
//      geoms NAG x [GEOM_I], pairs NPAIR x [2], equalities NEQ x [EQ_I],    geoms NAG x [GEOM_F], their solver parameters NAG x [GP_F],
//      frames NFRAME x [1], distances NDIST x [4], sensors NGS x [4],       equalities NEQ x [EQ_F], frames NFRAME x [FRAME_F], distances NDIST x [1]
//      the distances' geom lists                                          + reference frames at I[HI_REF]: [REF_F]
//    * pair tables at I[HI_PT]: [JH_PT_LEN]
//
// An offset slot that is zero says that the image has no such section.  EngineModel::init derives every offset; judo_amd/engine_model.py::image_offsets restates it.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstring>

#if defined(__HIPCC__)
#define JH_HD __host__ __device__
#else
#define JH_HD
#endif

void jh_set_error(const char* fmt, ...);

// The hand's pair tables (judo_amd/engine_model.py::hand_pair_tables, PT_*): [count, JH_PT_MAX records of JH_PT_I ints] at I[HI_PT].
constexpr int JH_PT_MAX = 4, JH_PT_I = 9, JH_PT_LEN = 1 + JH_PT_MAX * JH_PT_I;

namespace jh_eng {

constexpr int JFREE = 0, JSLIDE = 2, JHINGE = 3;
constexpr int GBOX = 6, GSPHERE = 2, GCAPSULE = 3, GCYLINDER = 5;
constexpr int HEADER_I = 24, HEADER_F = 24;
constexpr int BODY_I = 6, GEOM_I = 2, ACT_I = 2, BLOCK_I = 4, SENS_I = 3;
constexpr int BODY_F = 32, DOF_F = 20, ACT_F = 8, GEOM_F = 20, SITE_F = 3;
constexpr int EQ_I = 5, EQ_F = 12, FRAME_F = 12, GP_F = 8;  // GP: solref[2], solimp[5], pad
constexpr int LANES = 16, BODY_CODES = 20, BV_F = 8, REF_F = 16, GEN_I = 8;  // lane lists; hand bodies of the self-collision tables and floats per bounding volume; p_ref, R_ref, q_ref
// header ints: counts, integrator, cone; lane lists (offset, length of a list); generic block (ints, floats); body pairs, bounding volumes (floats), pairs; reference
// frames (floats); pair tables; the two words of diagnostic builds
enum { HI_NM = 0, HI_NBLK, HI_NV, HI_NQ, HI_NU, HI_NG, HI_NSITE, HI_NS, HI_INTEG, HI_CONE, HI_NSENS, HI_LANES, HI_LGM, HI_GI, HI_GF, HI_BP, HI_BS, HI_NBP, HI_REF, HI_PT, HI_ABLATE, HI_ABLATE_N };
// the generic block's own counts
enum { GI_NAG = 0, GI_NPAIR, GI_NEQ, GI_NFRAME, GI_NDIST, GI_NGS };
enum { EF_A0 = 0, EF_A1, EF_K, EF_B, EF_SOLIMP, EF_INVW = 9 };
// header floats
enum { HF_DT = 0, HF_IMPRATIO = 1, HF_TOL = 2, HF_MAXITER = 22, HF_LSTOL = 23, HF_GRAV = 3, HF_CK = 6, HF_CB = 7, HF_SOLIMP = 8, HF_CMASS = 13, HF_CINERTIA = 14, HF_CSIZE = 17, HF_CRBOUND = 20, HF_CTRAN = 21 };
// body floats
enum { BF_LPOS = 0, BF_LR = 3, BF_MASS = 12, BF_IPOS = 13, BF_IR = 16, BF_INERTIA = 25, BF_AXIS = 28, BF_TRAN = 31 };
// dof floats
enum { DF_DAMP = 0, DF_ARM, DF_FL, DF_FB, DF_FD, DF_INVW, DF_LIMITED, DF_LO, DF_HI, DF_LK, DF_LB, DF_SOLIMP, DF_FRCLIM = 16, DF_FRCLO, DF_FRCHI, DF_KV };
// actuator floats
enum { AF_KP = 0, AF_KV, AF_CLIM, AF_CLO, AF_CHI };
// geom floats
enum { GF_SIZE = 0, GF_POS = 3, GF_R = 6, GF_RBOUND = 15, GF_MU = 16 /* max(own, cube's) */, GF_TRAN = 17, GF_MUOWN = 18 };

struct EngineModel {  // views into a copy of the blob: the kernels' in LDS or global memory, the host's inside HostImage
  const float* F;
  const int* I;
  int NM, NBLK, NV, NQ, NU, NG, NSITE, NS, NSENS;
  int oBodyI, oBlockI, oActI, oGeomI, oSiteI, oSensI;
  int oBodyF, oDofF, oActF, oGeomF, oSiteF;
  // generic sections (reference kernel): all geoms incl. the cube, explicit pairs, equalities, frames, distance sensors
  int NAG, NPAIR, NEQ, NFRAME, NDIST, NGS, cone;
  int oAGI, oPairI, oEqI, oFrameI, oDistI, oSensG, oGlist, oAGF, oGPF, oEqF, oFrameF, oDistF;
  // Unchecked: the host calls it on an image that fits() and on no other.
  JH_HD void init(const float* f, const int* i) {
    F = f; I = i;
    NM = i[HI_NM]; NBLK = i[HI_NBLK]; NV = i[HI_NV]; NQ = i[HI_NQ]; NU = i[HI_NU]; NG = i[HI_NG]; NSITE = i[HI_NSITE]; NS = i[HI_NS]; NSENS = i[HI_NSENS];
    oBodyI = HEADER_I; oBlockI = oBodyI + NM * BODY_I; oActI = oBlockI + NBLK * BLOCK_I; oGeomI = oActI + NU * ACT_I;
    oSiteI = oGeomI + NG * GEOM_I; oSensI = oSiteI + NSITE;
    oBodyF = HEADER_F; oDofF = oBodyF + NM * BODY_F; oActF = oDofF + NV * DOF_F; oGeomF = oActF + NU * ACT_F; oSiteF = oGeomF + NG * GEOM_F;
    cone = i[HI_CONE];
    const int gi = i[HI_GI], gf = i[HI_GF];
    NAG = i[gi + GI_NAG]; NPAIR = i[gi + GI_NPAIR]; NEQ = i[gi + GI_NEQ]; NFRAME = i[gi + GI_NFRAME]; NDIST = i[gi + GI_NDIST]; NGS = i[gi + GI_NGS];
    oAGI = gi + GEN_I; oPairI = oAGI + NAG * GEOM_I; oEqI = oPairI + NPAIR * 2; oFrameI = oEqI + NEQ * EQ_I; oDistI = oFrameI + NFRAME;
    oSensG = oDistI + NDIST * 4; oGlist = oSensG + NGS * 4;
    oAGF = gf; oGPF = oAGF + NAG * GEOM_F; oEqF = oGPF + NAG * GP_F; oFrameF = oEqF + NEQ * EQ_F; oDistF = oFrameF + NFRAME * FRAME_F;
  }
  // Host: may init() run on the image of `nfloat` floats and `nint` ints at I, and may a reader index every section the view then names, and the leap family's
  // sections that the header slots name (the kernel of that family reads the slots itself; the host's names for them are HostImage's)?  True only if every count is
  // non-negative (NQ and NS, which size no section, within what NV, NM and NSENS allow: a joint per body, at most four values per sensor), every section ends inside
  // the image, and none begins in front of the end of the one before it in file order (an offset that points back into other records is refused, not followed).
  // The arithmetic is in 64 bits: a count of 0x7fffffff does not wrap.  Reads I alone, and nothing beyond what it has found to lie inside.
  bool fits(size_t nfloat, size_t nint) const {
    typedef long long L;
    const L nF = (L)nfloat, nI = (L)nint;
    if (nI < HEADER_I || nF < HEADER_F) return false;
    const L nm = I[HI_NM], nblk = I[HI_NBLK], nv = I[HI_NV], nq = I[HI_NQ], nu = I[HI_NU], ng = I[HI_NG], nsite = I[HI_NSITE], ns = I[HI_NS], nsens = I[HI_NSENS];
    if (nm < 0 || nblk < 0 || nv < 0 || nq < 0 || nu < 0 || ng < 0 || nsite < 0 || ns < 0 || nsens < 0 || nq > nv + nm || ns > 4 * nsens) return false;
    L eI = HEADER_I + nm * BODY_I + nblk * BLOCK_I + nu * ACT_I + ng * GEOM_I + nsite + nsens * SENS_I;  // (the ends of what has been checked so far)
    L eF = HEADER_F + nm * BODY_F + nv * DOF_F + nu * ACT_F + ng * GEOM_F + nsite * SITE_F;
    if (eI > nI || eF > nF) return false;
    const L ol = I[HI_LANES], lgm = I[HI_LGM];
    if (ol == 0 ? lgm != 0 : (ol < eI || lgm <= 0 || ol + LANES * lgm > nI)) return false;
    if (ol) eI = ol + LANES * lgm;
    const L obp = I[HI_BP], nbp = I[HI_NBP], obs = I[HI_BS];
    if (obp == 0 ? (nbp != 0 || obs != 0) : (obp < eI || nbp < 0 || obp + 2 * nbp + 2 * BODY_CODES > nI || obs < eF || obs + BODY_CODES * BV_F > nF)) return false;
    if (obp) { eI = obp + 2 * nbp + 2 * BODY_CODES; eF = obs + BODY_CODES * BV_F; }
    const L gi = I[HI_GI], gf = I[HI_GF];
    if (gi < eI || gi + GEN_I > nI || gf < eF || gf > nF) return false;
    const L nag = I[gi + GI_NAG], npair = I[gi + GI_NPAIR], neq = I[gi + GI_NEQ], nframe = I[gi + GI_NFRAME], ndist = I[gi + GI_NDIST], ngs = I[gi + GI_NGS];
    if (nag < 0 || npair < 0 || neq < 0 || nframe < 0 || ndist < 0 || ngs < 0) return false;
    const L odist = gi + GEN_I + nag * GEOM_I + npair * 2 + neq * EQ_I + nframe, oglist = odist + ndist * 4 + ngs * 4;
    eF = gf + nag * GEOM_F + nag * GP_F + neq * EQ_F + nframe * FRAME_F + ndist;
    if (oglist > nI || eF > nF) return false;
    for (L d = 0; d < ndist; d++) {  // a distance sensor's two geom lists: (first, count) twice, relative to the lists' start
      const int* di = I + odist + 4 * d;
      if (di[0] < 0 || di[1] < 0 || di[2] < 0 || di[3] < 0 || oglist + di[0] + (L)di[1] > nI || oglist + di[2] + (L)di[3] > nI) return false;
    }
    const L oref = I[HI_REF], opt = I[HI_PT];
    return (oref == 0 || (oref >= eF && oref + REF_F <= nF)) && (opt == 0 || (opt >= oglist && opt + JH_PT_LEN <= nI));
  }
};

// The host's view of an image it holds: the sections' sizes, whether the view fits them, and the view -- initialised only if it does.  The readers below and the
// launchers' acceptance tests ask `fits` before they index anything.  (F and I are set either way: the header slots of an image of HEADER_I ints can always be read.)
struct HostImage {
  EngineModel v = {};
  // the leap family's sections (0: the image has none): lane lists and a list's length, the hand's body pairs, per-body geom ranges and bounding volumes, the sensors' reference frames, the pair tables
  int oLane = 0, LGM = 0, oBP = 0, NBP = 0, oBG = 0, oBS = 0, oRef = 0, oPT = 0;
  size_t nfloat = 0, nint = 0;
  bool fits = false;
  void bind(const float* f, const int* i, size_t nf, size_t ni) {
    *this = HostImage{}; v.F = f; v.I = i; nfloat = nf; nint = ni;
    fits = v.fits(nf, ni);
    if (!fits) return;
    v.init(f, i);
    oLane = i[HI_LANES]; LGM = i[HI_LGM]; oBP = i[HI_BP]; NBP = i[HI_NBP]; oBG = oBP + 2 * NBP; oBS = i[HI_BS]; oRef = i[HI_REF]; oPT = i[HI_PT];
  }
};

// Cylinder geoms of an image that fits (type code GCYLINDER in the kernel's geom table): their number, or -1 with the error set when a record is malformed.  Only the
// leap family has a kernel that collides them (jh_engine_v5_cyl.hip); jh_model_create refuses them elsewhere.
inline int image_cylinders(const HostImage& im) {
  if (!im.fits) return 0;  // (not an engine image: the launchers refuse it)
  const EngineModel& v = im.v;
  int n = 0;
  for (long g = 0; g < v.NG; g++) {
    if (v.I[v.oGeomI + g * GEOM_I + 1] != GCYLINDER) continue;
    const float* f = v.F + v.oGeomF + g * GEOM_F;
    const float r = f[GF_SIZE], L = f[GF_SIZE + 1], rb = f[GF_RBOUND], want = sqrtf(r * r + L * L);
    if (!(r > 0.f) || !(L > 0.f) || f[GF_SIZE + 2] != 0.f) { jh_set_error("model_create: cylinder geom %ld: sizes must be (radius > 0, half length > 0, 0), got (%g, %g, %g)", g, r, L, f[GF_SIZE + 2]); return -1; }
    if (!(fabsf(rb - want) <= 1e-5f * want)) { jh_set_error("model_create: cylinder geom %ld: bounding radius %g is not sqrt(r^2 + L^2) = %g", g, rb, want); return -1; }
    n++;
  }
  return n;
}

// Arm pairs of an fr3_pick image that fits (the generic block: geom records, then the candidate pairs): the pairs between two moving bodies of the arm (body
// codes >= 1) other than finger against finger (bodies 8 and 9), plus those of a box or a capsule on the arm against a capsule of the static geometry (the fr3_link0 stand-in) -- what the
// default build of k_fr3_v6 leaves out and its self-collision build (jh_engine_v6_self.hip) collides.  -1 with the error set when a pair record is malformed: behind a
// model_create that succeeded, every pair of an image that fits names two different geoms of the block (jh_model_is_fr3 indexes with them).
inline int image_arm_pairs(const HostImage& im) {
  constexpr int LF = 8, RF = 9;
  if (!im.fits) return 0;  // (not an engine image: the launchers refuse it)
  const EngineModel& v = im.v;
  const int* I = v.I;
  const long nag = v.NAG;
  int n = 0;
  for (long p = 0; p < v.NPAIR; p++) {
    const long g1 = I[v.oPairI + 2 * p], g2 = I[v.oPairI + 2 * p + 1];
    if (g1 < 0 || g1 >= nag || g2 < 0 || g2 >= nag || g1 == g2) { jh_set_error("model_create: candidate pair %ld names geoms (%ld, %ld) of %ld", p, g1, g2, nag); return -1; }
    const int b1 = I[v.oAGI + g1 * GEOM_I], t1 = I[v.oAGI + g1 * GEOM_I + 1], b2 = I[v.oAGI + g2 * GEOM_I], t2 = I[v.oAGI + g2 * GEOM_I + 1];
    const bool arm_arm = b1 >= 1 && b2 >= 1 && !((b1 == LF && b2 == RF) || (b1 == RF && b2 == LF));
    const bool arm_capsule = t1 == GCAPSULE || (t1 == GBOX && t2 == GCAPSULE && b1 >= 1);  // (a capsule of the arm or of the static base against the arm)
    if (!arm_arm && !arm_capsule) continue;
    if (b1 == b2) { jh_set_error("model_create: candidate pair %ld collides two geoms of arm body %d with each other", p, b1); return -1; }
    if (t1 == GCAPSULE && t2 != GCAPSULE) { jh_set_error("model_create: candidate pair %ld between arm bodies has its capsule first; the kernel takes (box, capsule)", p); return -1; }
    n++;
  }
  return n;
}

// The pair tables of a leap image (the hand's broad phase, jh_engine_v5.hip): I[HI_PT] is the offset of [count, JH_PT_MAX records of JH_PT_I ints] behind everything else
// in the int section, 0 in an image without them.  Ints of the block (0: none), or -1 with the error set when it is malformed: the kernel indexes lanes and
// pair bits with what the records hold.  Reads the header and the block alone, which it bounds itself: asked of every leap image, whether the view fits or not.
inline int image_pair_tables(const HostImage& im) {
  const int* I = im.v.I;
  if (im.nint < (size_t)HEADER_I || I[HI_PT] == 0) return 0;
  const long o = I[HI_PT], len = JH_PT_LEN, nbp = I[HI_NBP];
  if (o < HEADER_I || o + len > (long)im.nint) { jh_set_error("model_create: the pair tables at int %ld (%ld ints) lie outside the int section of %u", o, len, (unsigned)im.nint); return -1; }
  const int n = I[o];
  if (n < 0 || n > JH_PT_MAX) { jh_set_error("model_create: %d pair tables, at most %d", n, JH_PT_MAX); return -1; }
  for (int t = 0; t < JH_PT_MAX; t++) {
    const int* T = I + o + 1 + t * JH_PT_I;
    if (t >= n) { for (int k = 0; k < JH_PT_I; k++) if (T[k] != 0) { jh_set_error("model_create: pair table %d is beyond the count of %d and not zero", t, n); return -1; } continue; }
    float f[4]; memcpy(f, T + 3, sizeof(f));
    if (T[0] < 0 || T[0] >= nbp || (t > 0 && T[0] <= T[-JH_PT_I])) { jh_set_error("model_create: pair table %d names body pair %d of %ld (ascending, each once)", t, T[0], nbp); return -1; }
    if (T[1] < 0 || T[1] >= LANES || T[2] < 0 || T[2] >= LANES) { jh_set_error("model_create: pair table %d names joints (%d, %d) of %d", t, T[1], T[2], LANES); return -1; }
    if (!std::isfinite(f[0]) || !std::isfinite(f[2]) || !std::isfinite(f[1]) || !std::isfinite(f[3]) || !(f[1] > 0.f) || !(f[3] >= 0.f)) {
      jh_set_error("model_create: pair table %d: grid origins (%g, %g) and inverse cell widths (%g, %g) must be finite, the first width positive", t, f[0], f[2], f[1], f[3]);
      return -1;
    }
  }
  return (int)len;
}

// May two images of one model set share the pair tables in the set's int section?  Only if the tables are the same words and everything they were computed from is:
// the hand bodies' frames and joint axes, the joint ranges, every hand geom's size and pose, the bodies' bounding volumes.  (The cube, masses, gains and friction
// are free to differ.)  Images without tables share "none".  `b` is read at the offsets of `a`, inside sections of a's sizes.
inline bool pair_tables_shared(const HostImage& a, const HostImage& b) {
  const int *I0 = a.v.I, *I = b.v.I;
  const float *F0 = a.v.F, *F = b.v.F;
  if (a.nint <= (size_t)HI_PT || b.nint != a.nint || b.nfloat != a.nfloat || I[HI_PT] != I0[HI_PT]) return false;
  const long o = I0[HI_PT], len = JH_PT_LEN;
  if (o == 0) return true;
  if (o < HEADER_I || o + len > (long)a.nint || memcmp(&I[o], &I0[o], 4 * len) != 0) return false;
  const EngineModel& v = a.v;
  if (!a.fits || v.NM < 1 || v.NV < 6 || a.oBP == 0) return false;
  auto same = [&](long at, long n) { return memcmp(&F[at], &F0[at], 4 * n) == 0; };
  for (long k = 1; k < v.NM; k++) if (!same(v.oBodyF + k * BODY_F + BF_LPOS, 12) || !same(v.oBodyF + k * BODY_F + BF_AXIS, 3)) return false;  // frame in the parent (position, rotation), joint axis
  for (long d = 6; d < v.NV; d++) if (!same(v.oDofF + d * DOF_F + DF_LIMITED, 3)) return false;                                              // limited, range
  for (long g = 0; g < v.NG; g++) if (!same(v.oGeomF + g * GEOM_F, GF_RBOUND + 1)) return false;                                              // size, position, rotation, bounding radius
  return same(a.oBS, BODY_CODES * BV_F);                                                                                                      // bounding sphere and box per hand body
}

}  // namespace jh_eng
