// jh_engine_v5.hip -- leap_cube rollout kernel, second cooperative generation (gfx950): the arithmetic of jh_engine_v2.hip on a register
// diet, so that more than one wave fits on a SIMD.
//
// jh_engine_v2.hip runs one wave per SIMD (487 registers) and is stalled ~75 % of the time on dependent VALU / LDS / DPP chains with
// nothing to switch to.  Same decomposition here -- 16 lanes (one DPP row) per rollout, lane (c,s) owns link s of finger chain c, its
// joint, its actuator, its dof rows and <= 2 contacts -- but everything a lane does not need in every instruction lives in LDS:
//   * per-lane model constants, the lane's spline knots, the warm start, the chain inertia blocks;
//   * a contact slot keeps frame (9), lever arm (3), cone constants (5), aref / jar / jp (9): the finger-side Jacobian columns are
//     recomputed from the joint axes / anchors in LDS wherever they are used (J x, J'f, J'WJ), the cube-side rotational columns from the
//     lever arm and the cube rotation;
//   * every contact contribution to the gradient and to the arrow Hessian is an LDS float atomic (the cube block as well: no 21-entry
//     register partials and no 21 row sums per iteration); row sums remain only for the scalars of the convergence test and line search;
//   * the cube-chain coupling Y = L^-1 Hcb is spread over the chain's four lanes (<= 2 of the 6 columns per lane) instead of being held
//     whole by every lane; the Schur-complement dot products are shared the same way.
// The solver itself (primal Newton, exact line search, warm start, termination) is unchanged: results agree with jh_engine_v2.hip to
// summation order, and the parity suite (tests/test_gpu_leap.py) runs against both.
#include <cstddef>
#include <type_traits>

#include "jh_coop.h"

using namespace jh_eng;
using namespace jh_coop;

namespace {

#ifdef JH_V5_WAVESTAMP
__device__ unsigned long long* g_wavestamp = nullptr;  // six words per group of four rollouts (see the kernel); set by jh_v5_wavestamp_buffer
__device__ int g_wavestamp_cap = 0;
#endif

constexpr int G = 16, RPW = 4, WAVE = 64;
constexpr int NCH = 4, NLK = 4;
// ---- The Newton iteration's formulation (round 4).  The alternatives below were A/B-measured on the recorded plan inputs within one GPU box each
// (profiles/r04_leap_experiments.txt) and then taken out of the source (the git history has them as JH_V5_* switches):
//  * gradient and Hessian of an iterate from ONE pass over the contacts (joint columns, world force and cone weights computed once, one fence less) instead of a gradient pass,
//    the convergence test, and a Hessian pass that re-used the cone weights: 69.1 -> 68.2 ms, same iterates bit for bit;
//  * the cube block of J'WJ (21 entries) and the cube part of -J'f (6) as sums over the rollout's lanes instead of LDS float atomics: every cube contact of a rollout adds to
//    the same addresses and same-address atomics serialise: 68.2 -> 64.5 ms.  (With packed-fp32 code, rounds 2-3, six atomics for the gradient were 1 % faster than six row
//    sums; without the SLP vectorizer the row sums are 1.7 % faster.)  Cost probes on the atomics that remain -- the instruction issued twice, the second adding zero -- put the
//    24 Hcb atomics of a contact at 3.4 % and the 10 Hbb ones at 1.4 % of the kernel;
//  * the 27 sums as two 16-value reduce-scatters (jh_coop.h row_scatter16: lane l receives entry l; 45 instructions per 16 sums instead of 80): 61.85 -> 61.25 ms;
//  * the Schur complement Hcc - sum over chains of Y'Y never goes back to the LDS: the four chains' terms are summed with qsum4_same, whose result is bit-identical in every
//    lane, and each lane subtracts them from the assembled block with 27 quad broadcasts: 64.6 -> 63.4 ms.  Earlier forms: `S.Hcc[..] -= da` (every read-modify-write its own
//    LDS round trip, fourteen in a row), LDS atomics by the first chain's lanes (79.4 -> 78.4 ms), by every chain's lanes (+9.7 %).  With qsum4's association, which differs
//    from chain to chain, the lanes of a rollout solved four slightly different 6 x 6 systems: +0.3 % iterations and 2 000 rollout-steps at the iteration cap;
//  * J'WJ from world-frame dof columns and A = Fr' W Fr (one symmetric 3 x 3 per contact; the cube's translation columns are unit vectors) instead of frame-space columns
//    times W: 63.3 -> 61.7 ms;
//  * two surviving hand body pairs per level-2 broad-phase pass when both have at most 8 geoms: never applies (the survivors involve the palm's geom groups), +0.8 %.
// Measured since and taken out the same way:
//  * a line search that, where the safeguarded Newton search is in trouble, tries the step lengths at which the slope jumps (a friction-loss row's zero crossing, a contact's
//    friction reversal): 3.65 instead of 4.68 slope evaluations per Newton iteration of a wave, the 9..16-evaluation searches gone (15 % -> 3 % of the searches), and the
//    kernel 2.1 % SLOWER (82.45 against 80.75 ms): an evaluation is ~1 % of an iteration's issue slots, the candidates' registers and the extra block cost more than a fifth of
//    them (profiles/r04_leap_experiments.txt; no gain on the round-6 kernel either, profiles/r06_experiments.txt);
//  * a third copy of the constraint rows + solver with ONE slot per lane for the wave-steps in which no rollout has more than 16 contacts: 93 % of the wave-steps qualify and
//    the kernel is 1.1 % faster (79.7 against 80.6 ms), but the copies contract differently, so a rollout's bits depend on its wave-mates (test_leap_full_size_properties
//    fails); under -ffp-contract=on, bit-identical and +-0.2 % (profiles/r04_leap_experiments.txt, profiles/r06_experiments.txt);
//  * the joints above a link visited one by one, each under its own `j <= depth` test, instead of link_c3's batch: 71.8 against 70.0 ms without the SLP vectorizer (with
//    packed-fp32 code, rounds 2-3, the batch was the slower form, 83.0 against 79.4 ms: no room for 24 joint floats beside the packed operands' register pairs);
//  * the line search's Newton step with the correctly rounded division (10 instructions per evaluation) instead of v_rcp_f32: +0.2 %;
//  * OPAQUE on a contact slot's frame as well as its sides and lever arm, or again before the Hessian assembly and the line search: 71.6 and 71.0 against 70.0 ms (with the
//    hand's own contacts and packed-fp32 code, rounds 2-3, the frame paid); the lane id left transparent at the top of the step loop: 73.6 against 70.0 ms; the step-level state
//    held across the Newton loop instead of parked in LDS: 71.7 against 71.4 ms (all profiles/r04_leap_experiments.txt);
//  * the lane's spline knots staged in LDS, at most 8 per actuator (the round-1..3 layout), and round 3's occupancy experiments on the cube-only instantiations -- the hand's
//    arrays shrunk to stubs, the per-rollout LDS hidden from the compiler, a fixed register budget: DESIGN.md section 5.1, profiles/r03_leap_occupancy_experiment.txt;
//  * the joint columns of the first slot's side-B link recomputed at every use instead of cached per step: 59.3 against 58.3 ms, the same iterates bit for bit
//    (profiles/r05_leap_experiments.txt);
//  * the kernel without its trace rows, a probe of what re-rolling the E <= 5 elites instead would save in this launch: profiles/r05_trace_ab.txt;
//  * the cube's rotation solved in the body frame (rotation columns (R e_q) x r, a 3 x 3 product wherever they are used): 58.0-58.2 against 57.5-57.6 ms; the hand-capable
//    copy's chain part with an exec-masked region per joint and per coupling, or with the coupling of a contact off the cube added as zeros (profiles/r06_experiments.txt);
//  * the hand's broad phase with one box-test pass per 16 body PAIRS (7 or 8 passes, a few lanes each) and one level-2 trip per near geom of side A with only B's near lanes at
//    work: the same candidate list entry for entry, in more and emptier passes (profiles/leap_broad_phase.md).

// ---- tuning constants
constexpr int LSMAX = 16;           // slope evaluations per line search at the most (12 and 20: no gain, profiles/r06_experiments.txt)
constexpr int WAVES_PER_EU = 2;     // the kernel's launch bound: the register budget of two waves per SIMD
constexpr int WAVES_PER_BLOCK = 4;  // waves per workgroup: they share one LDS copy of the model image and nothing else
constexpr int BFS = 33;             // row stride of the LDS copy of the body records (BODY_F = 32 floats each): odd, the four chains' rows in different banks
constexpr int PAS = 9;              // row stride of S.pa
constexpr int RSPAD = 4;            // floats behind an RS record (see its last member)
constexpr int C3PAD = 278;          // floats in front of the c3 cache inside the pool's storage (see RS)
constexpr int NSLDS = 3;            // slots per lane whose contacts the LDS pool holds
constexpr double BIGPROB = 0.999999;  // how sure the compiler may be that a wave-step stays on the NSLOT copy (block frequencies steer the placement of register spills)
// Waves of a workgroup never exchange data after the image is staged: inside the step loop a "barrier" only has to order one wave's own LDS traffic
// (a wave's LDS instructions execute in issue order), so it is a compiler fence, not an s_barrier -- rollouts in different waves never wait for each other.
// OPAQUE(x): the compiler forgets what it knows about x, so nothing derived from it is hoisted out of the enclosing loop.  Used on the contact slots at the top of
// every Newton iteration: otherwise the slots' Jacobian columns, lever arms and LDS addresses (all invariant over the iterations) are computed once before
// the loop, do not fit in the register file and are spilled and reloaded in every iteration.
#define OPAQUE(x) asm volatile("" : "+v"(x))
// The parked state of a horizon slice (see the kernel): PARK_F floats per queue unit, every word stored and loaded at device scope
constexpr int PARK_F = 5 * 64;
// An explicit schedule of horizon slices (jh_model_set_rollout_slice_bounds, and the automatic taper): sixteen 16-bit step indices, two to a word, passed to the kernel by
// value -- entry s is the step behind slice s's last, entries from the last slice on hold H -- and read from the kernel arguments with a uniform load, once per unit.
// A batched launch has no queue and no slices: when it has a controller axis (jh_plan_step_ensemble_batch) the same eight words carry that axis's three strides --
// block, noise, image, in floats, each as a low and a high word -- so the kernel's argument list, and with it the argument offsets of every other instantiation, stays
// what it was.
struct SliceBounds { unsigned w[8]; };
__host__ __device__ inline long long axis_stride(const SliceBounds& sb, int i) { return (long long)(((unsigned long long)sb.w[2 * i + 1] << 32) | sb.w[2 * i]); }
inline void set_axis_stride(SliceBounds& sb, int i, long long v) { sb.w[2 * i] = (unsigned)((unsigned long long)v & 0xffffffffull); sb.w[2 * i + 1] = (unsigned)((unsigned long long)v >> 32); }
// The batched instantiations' last argument: those eight words and, behind them, the plant axis (jh_internal.h: the rollout-index stride and the table that maps a
// problem to its image).  A type of its own for BATCH alone, so that every other instantiation keeps the argument block it had, byte for byte.
struct BatchBounds : SliceBounds { jh_plant_axis plants; };
constexpr int MAX_BOUND_SLICES = 16;
#define PARK_LD(p) __hip_atomic_load((p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
#define PARK_ST(p, v) __hip_atomic_store((p), (v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
#define WSYNC() do { __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront"); } while (0)
#ifndef JH_V5_NSLOT
#define JH_V5_NSLOT 2
#endif
#ifndef JH_V5_NSBIG
#define JH_V5_NSBIG 3  // 4: 64 contacts, the 16 above the LDS pool in a row of global memory (as jh_engine_v6.hip does): 0 instead of 1.7e-6 contacts dropped per rollout-step on the
                       // recorded headline inputs and 97 % instead of 91 % of the jammed-cube sweep inside the capacity, for +2.8 % on every plan step (81.0 against 78.8 ms): not the default
#endif
#ifndef JH_V5_CYL
#define JH_V5_CYL 0  // 1 (jh_engine_v5_cyl.hip): the build for an image that keeps caltech_leap_cube's fingertip cylinders (geom type 5: radius, half length along the geom's z).
                     // Sphere against cylinder is MuJoCo's primitive; box and cylinder against cylinder go through the bounded fp32 GJK + EPA of jh_coop.h, a call that is
                     // not inlined and keeps its polytope in the lane's private memory -- behind a test that only a lane with such a pair passes.  0: no line of it is compiled.
#endif
constexpr int GCYL = 5;
constexpr int NSLOT = JH_V5_NSLOT;  // contact slots per lane of the common case: steps with at most 16 * NSLOT contacts in every rollout of the wave
constexpr int NSBIG = JH_V5_NSBIG;  // ... of the rare case (6e-4 of the rollout-steps of the headline workload): the wave runs a second copy of the solver with this many slots
constexpr int NCP = 16 * (NSBIG < NSLDS ? NSBIG : NSLDS);  // contact pool per rollout in LDS
constexpr int NCAP = 16 * NSBIG;                           // contacts a rollout can hold: those above the LDS pool live in its row of the global overflow pool
constexpr int NOVF = NCAP - NCP;
constexpr int MAXHIT = 64;  // broad-phase survivors (candidate geom pairs) per rollout and step; 16 bits each.  More than that are counted as dropped contacts
constexpr int POOL_F = 10;  // pos3, normal3, dist, mu, body, tran
constexpr int MAXG = 80, MAXLG = 8;
constexpr int CUBE = 17;          // contact side codes: 0 = static geometry, 1..16 = finger link (1 + 4*chain + depth), 17 = the cube
constexpr int HITPAIR = 1 << 15;  // broad-phase survivors >= HITPAIR are hand-hand geom pairs (ga << 7 | gb, geom ids < 128), smaller ones are cube-vs-geom
static_assert(MAXG <= 128, "hand geom pairs are packed into 14 bits");
constexpr int MAXBP = 128;         // hand body pairs in the model image (leap_cube 106, caltech_leap_cube 122)
constexpr int PT_MAX = JH_PT_MAX, PT_I = JH_PT_I;  // pair tables of the hand's broad phase: at most four, nine ints each (pair, the two joints' lanes, grid origins and inverse cell widths as float bits, the 64-bit word)
constexpr int MAXBPL = 96;        // hand body pairs whose bounding volumes overlap, per rollout and step (one byte each: pair indices < MAXBP <= 256)
constexpr int NDH = 22 * 23 / 2;  // dense Hessian (packed lower) of a rollout whose contacts couple two finger chains
constexpr int NV = 22, NQ = 23, NU = 16, NS = 31, NS_CALTECH = 23, NX = 45, NMB = 17;
constexpr int NBC = BODY_CODES;  // hand bodies of the self-collision tables: 0 = static geometry, 1..16 = finger links, 17..19 = further groups of static geometry (engine_model.py)
__device__ __forceinline__ bool static_code(int b) { return b == 0 || b >= NMB; }

// per-lane model constants staged in LDS (index = lane & 15)
enum { LC_DAMP = 0, LC_KVD, LC_KP, LC_KV, LC_CLO, LC_CHI, LC_CLIM, LC_FL, LC_FB, LC_FD, LC_INVW, LC_LIMITED, LC_LO, LC_HI, LC_LK, LC_LB, LC_SI, LC_IMCK = LC_SI + 5, LC_N = 25 };  // (LC_IMCK: 1 / (the cube's mass or inertia of dof l), lanes 0..5; zero elsewhere)  // (row stride of the LDS table: odd, so that the 16 lanes' rows start in 16 different banks)

struct __attribute__((aligned(16))) RS {  // per-rollout shared state in LDS
  float pa[NMB][PAS];   // body origin (0..2) and joint axis in the world (4..6); odd row stride: lanes reading 16 different bodies hit 16 different banks
  float xR[NMB][9];
  float qv[NV], g[NV], p[NV], ws[NV];
  float acn[6];       // constraint-consistent cube acceleration of this step (every lane integrates the replicated cube state)
  float Mbb[NCH][10];
  float rhs6[6];
  float cmd[4];      // the cube's mass and its three principal inertias: the diagonal of its mass block, next to rhs6 so that the Schur step's reads bring it along
  union {
    struct {
      float bs[NBC][4];   // bounding sphere of the hand bodies (0, 17.. = static geometry, 1..16 = finger links): world centre, radius (the centre is the
                          // bounding box's too; its half sizes and axes come from the model image and the body rotation)
      unsigned short hits[MAXHIT];
      unsigned char bpl[MAXBPL];
    };
    // the collision arrays are dead from the constraint rows on: the step-level state the Newton loop does not touch is parked here instead of being held in
    // registers (or spilled to scratch memory by the compiler) across the loop.  The joint velocity and the cube's velocity are in qv already.
    struct { float pk_q[G], pk_fs[G], pk_cq[4], pk_acc; };
  };
  union {  // the contact pool is dead once every lane has loaded its slots; the Newton Hessian then reuses its storage
    float pool[NCP][POOL_F];
    struct { float Hcc[21], Hbb[NCH][10], Hcb[NCH][24], Hx[6][16]; };  // Hcb[c][j*6+q]: chain column j, cube row q; Hx[pidx(a,b)][ib*4+ia]: block (chain b, chain a)
                                                                       // of a contact-coupled pair of chains a < b (hand self-collision)
    struct { float Hd[NDH], dinv[NV]; };                    // dense path (contacts between two finger chains): packed lower 22 x 22, reciprocal pivots
    struct { float c3pad_[C3PAD]; float c3s[G][12]; };   // behind the Newton matrices (275 floats at most): the first slot's joint columns, per lane; 16-byte aligned rows (static_assert below)
  };
  int ncon, nhit;
  float pad_[RSPAD];  // record size = 16 banks modulo 64: the same field of a wave's four rollouts starts in four disjoint groups of 16 banks
};

static_assert(offsetof(RS, c3s) % 16 == 0 && C3PAD >= NDH + NV && sizeof(((RS*)nullptr)->c3pad_) + sizeof(((RS*)nullptr)->c3s) <= sizeof(((RS*)nullptr)->pool), "c3 cache: aligned rows behind the Newton matrices, inside the pool's storage");
struct PoolCtx { RS* S; int* overflow; float* ovf; };  // ovf: this rollout's row of the global overflow pool (NOVF x POOL_F floats), or null

__device__ __forceinline__ void push_contact(const PoolCtx& pc, const float* pos, const float* n, float dist, int body, float mu, float tran) {
  int i = atomicAdd(&pc.S->ncon, 1);
  float* e;
  if (i < NCP) e = pc.S->pool[i];
  else if (NOVF > 0 && pc.ovf && i < NCAP) e = pc.ovf + (i - NCP) * POOL_F;
  else { if (pc.overflow) atomicAdd(pc.overflow, 1); return; }
  e[0] = pos[0]; e[1] = pos[1]; e[2] = pos[2]; e[3] = n[0]; e[4] = n[1]; e[5] = n[2]; e[6] = dist; e[7] = mu; e[8] = __int_as_float(body); e[9] = tran;
}

struct LeapSink {  // contacts of one geom pair: sides packed as A | B << 8; `flip`: the narrow phase ran with the two geoms swapped (normal B -> A)
  PoolCtx pc; int sides; float mu, tran; bool flip;
  __device__ __forceinline__ void push(const float* pos, const float* n, float dist) {
    const float nn[3] = {flip ? -n[0] : n[0], flip ? -n[1] : n[1], flip ? -n[2] : n[2]};
    push_contact(pc, pos, nn, dist, sides, mu, tran);
  }
};

#if JH_V5_CYL
struct CvxOne {  // the one contact of collide_convex_cylinder
  float pos[3], n[3], dist; bool hit;
  __device__ __forceinline__ void push(const float* p, const float* nn, float d) { for (int k = 0; k < 3; k++) { pos[k] = p[k]; n[k] = nn[k]; } dist = d; hit = true; }
};
#endif

// ------------------------------------------------------------------------------------------------ per-lane contact slot (27 registers)
struct Slot {
  int la, lb;        // the two sides (normal from A to B): la = -1 empty slot; 0 = static geom, 1 + 4*chain + depth = finger link, CUBE
  float fr[9];       // contact frame rows (normal, t1, t2), world
  float rc[3];       // contact point relative to the cube origin, world
  float aref[3], D0, D1, Dm, mu, fri;
  float jar[3], jp[3];
};

// two oriented boxes (centre, rotation, half sizes): false when one of the six face axes separates them (a conservative cull: the nine edge axes are
// left to the narrow phase)
__device__ __forceinline__ bool obb_face_overlap(const float* ca, const float* Ra, const float* ha, const float* cb, const float* Rb, const float* hb) {
  const float d[3] = {cb[0] - ca[0], cb[1] - ca[1], cb[2] - ca[2]};
  float C[9];  // C = |Ra' Rb|
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 3; j++) C[3 * i + j] = fabsf(Ra[i] * Rb[j] + Ra[3 + i] * Rb[3 + j] + Ra[6 + i] * Rb[6 + j]);
  bool ok = true;
#pragma unroll
  for (int i = 0; i < 3; i++) {
    const float da = fabsf(d[0] * Ra[i] + d[1] * Ra[3 + i] + d[2] * Ra[6 + i]);
    ok = ok && da <= ha[i] + hb[0] * C[3 * i] + hb[1] * C[3 * i + 1] + hb[2] * C[3 * i + 2];
    const float db = fabsf(d[0] * Rb[i] + d[1] * Rb[3 + i] + d[2] * Rb[6 + i]);
    ok = ok && db <= hb[i] + ha[0] * C[i] + ha[1] * C[3 + i] + ha[2] * C[6 + i];
  }
  return ok;
}

// index of the k-th set bit (k = 0: the lowest) of a 16-bit mask with more than k bits set: four halvings on the population count, no loop and no table
__device__ __forceinline__ int nth_bit16(unsigned m, int k) {
  int pos = 0, c = __popc(m & 0xFFu);
  bool up = k >= c; k = up ? k - c : k; m = up ? m >> 8 : m; pos = up ? 8 : 0;
  c = __popc(m & 0xFu); up = k >= c; k = up ? k - c : k; m = up ? m >> 4 : m; pos = up ? pos + 4 : pos;
  c = __popc(m & 0x3u); up = k >= c; k = up ? k - c : k; m = up ? m >> 2 : m; pos = up ? pos + 2 : pos;
  return k >= (int)(m & 1u) ? pos + 1 : pos;
}
#ifdef JH_V5_COUNT
__device__ __forceinline__ int wave_rowmax(int v) {  // the maximum over the wave's four rows of a value that is uniform within a row
  return max(max(__builtin_amdgcn_readlane(v, 0), __builtin_amdgcn_readlane(v, 16)), max(__builtin_amdgcn_readlane(v, 32), __builtin_amdgcn_readlane(v, 48)));
}
#endif

// The three functions below visit the joints above a finger link.  All four joints of the chain are loaded and their columns axis_j x (pos - anchor_j) computed
// UNCONDITIONALLY (link_c3), the depth of the link only masks what is accumulated.  A per-joint form (`if (j <= dep) { load; compute; }`) puts every joint's LDS loads under
// its own exec mask, so each of them is a round trip of its own -- 50 of the 80 `s_waitcnt lgkmcnt(0)` of a Newton iteration sat in these loops; the batched form waits once
// per call and has no branches (the wasted columns of the shallower links are cheaper than the waits).  Same expressions: same bits.
__device__ __forceinline__ void link_c3(const RS& S, int ch, const float* pos, float (*c3)[3]) {
#pragma unroll
  for (int j = 0; j < NLK; j++) {
    const float* pj = S.pa[1 + 4 * ch + j];
    const float rb[3] = {pos[0] - pj[0], pos[1] - pj[1], pos[2] - pj[2]};
    cross3(c3[j], pj + 4, rb);
  }
}
__device__ __forceinline__ void load_c3(const float* c3c, float (*c3)[3]) {
  const float4 a = *reinterpret_cast<const float4*>(c3c), b = *reinterpret_cast<const float4*>(c3c + 4), c = *reinterpret_cast<const float4*>(c3c + 8);
  c3[0][0] = a.x; c3[0][1] = a.y; c3[0][2] = a.z; c3[1][0] = a.w; c3[1][1] = b.x; c3[1][2] = b.y; c3[2][0] = b.z; c3[2][1] = b.w; c3[2][2] = c.x; c3[3][0] = c.y; c3[3][1] = c.z; c3[3][2] = c.w;
}
// velocity of the point `pos` carried by finger link `code` for the joint-rate vector `vec` (22-vector in LDS), times `sign`, added to w
// (c3c: the lane's cached columns of this link and point -- the c3 cache, S.c3s -- or null)
__device__ __forceinline__ void link_vel(const RS& S, int code, const float* pos, const float* vec, float sign, float* w, const float* c3c = nullptr) {
  const int ch = (code - 1) >> 2, dep = (code - 1) & 3;
  float c3[NLK][3]; if (c3c) load_c3(c3c, c3); else link_c3(S, ch, pos, c3);
#pragma unroll
  for (int j = 0; j < NLK; j++) {
    const float vj = vec[6 + 4 * ch + j];  // (loaded whatever the depth: a valid address, and a conditional load is an exec-mask round trip)
    const float xj = j <= dep ? sign * vj : 0.f;
    w[0] = fmaf(c3[j][0], xj, w[0]); w[1] = fmaf(c3[j][1], xj, w[1]); w[2] = fmaf(c3[j][2], xj, w[2]);
  }
}
// -J'F for the joints of finger link `code` (F = world force on side B; sign = +1 for side B, -1 for side A): LDS float atomics into g
__device__ __forceinline__ void link_force(RS& S, int code, const float* pos, const float* Fw, float sign) {
  const int ch = (code - 1) >> 2, dep = (code - 1) & 3;
  float c3[NLK][3]; link_c3(S, ch, pos, c3);
  float v[NLK];
#pragma unroll
  for (int j = 0; j < NLK; j++) v[j] = -sign * dot3(c3[j], Fw);
#pragma unroll
  for (int j = 0; j < NLK; j++) if (j <= dep) atomicAdd(&S.g[6 + 4 * ch + j], v[j]);
}
// Jacobian columns (contact frame) of the joints of finger link `code`, times `sign`, added to Jb[j] (j = depth in the chain)
__device__ __forceinline__ void link_cols(const RS& S, int code, const float* pos, const float* fr, float sign, float (*Jb)[3]) {
  const int ch = (code - 1) >> 2, dep = (code - 1) & 3;
  float c3[NLK][3]; link_c3(S, ch, pos, c3);
#pragma unroll
  for (int j = 0; j < NLK; j++) {
    const float sg = j <= dep ? sign : 0.f;
    Jb[j][0] = fmaf(sg, dot3(fr, c3[j]), Jb[j][0]); Jb[j][1] = fmaf(sg, dot3(fr + 3, c3[j]), Jb[j][1]); Jb[j][2] = fmaf(sg, dot3(fr + 6, c3[j]), Jb[j][2]);
  }
}

// contact-frame image of the relative point velocity (side B minus side A) for the generalised velocity whose cube part is (xl = linear, world;
// wang = R_cube * angular part, world) and whose finger part is `vec` (22-vector in LDS)
template <bool SELF>
__device__ __forceinline__ void slot_Jx(const Slot& s, const RS& S, const float* qcpos, const float* xl, const float* wang, const float* vec, float* out, const float* c3c = nullptr) {
  float w[3] = {0.f, 0.f, 0.f};
  const float pos[3] = {s.rc[0] + qcpos[0], s.rc[1] + qcpos[1], s.rc[2] + qcpos[2]};
  if (!SELF || s.la == CUBE) { float wx[3]; cross3(wx, wang, s.rc); w[0] = -(xl[0] + wx[0]); w[1] = -(xl[1] + wx[1]); w[2] = -(xl[2] + wx[2]); }
  else if (SELF && s.la > 0) link_vel(S, s.la, pos, vec, -1.f, w);
  if (s.lb > 0) link_vel(S, s.lb, pos, vec, 1.f, w, c3c);
  out[0] = dot3(s.fr, w); out[1] = dot3(s.fr + 3, w); out[2] = dot3(s.fr + 6, w);
}

// slot_Jx for a cube contact of the copy without the hand's own contacts, FIRST slot, without a branch: the finger part is computed whatever the slot holds (an empty slot or a
// contact between the cube and the static geometry reads valid addresses -- link code 0 gives chain -1, entries 2..5 of `vec`) and dropped by a select; an empty slot's frame is
// zero, so its image is zero.  The same fused multiply-adds in the same order as slot_Jx: same bits.
__device__ __forceinline__ void slot_Jx_first(const Slot& s, const float* xl, const float* wang, const float* vec, float* out, const float* c3c) {
  float wx[3]; cross3(wx, wang, s.rc);
  const float w0[3] = {-(xl[0] + wx[0]), -(xl[1] + wx[1]), -(xl[2] + wx[2])};
  const int ch = (s.lb - 1) >> 2, dep = (s.lb - 1) & 3;
  float c3[NLK][3]; load_c3(c3c, c3);
  float w[3] = {w0[0], w0[1], w0[2]};
#pragma unroll
  for (int j = 0; j < NLK; j++) {
    const float vj = vec[6 + 4 * ch + j];
    const float xj = j <= dep ? vj : 0.f;
    w[0] = fmaf(c3[j][0], xj, w[0]); w[1] = fmaf(c3[j][1], xj, w[1]); w[2] = fmaf(c3[j][2], xj, w[2]);
  }
  const bool lk = s.lb > 0;
  w[0] = lk ? w[0] : w0[0]; w[1] = lk ? w[1] : w0[1]; w[2] = lk ? w[2] : w0[2];
  out[0] = dot3(s.fr, w); out[1] = dot3(s.fr + 3, w); out[2] = dot3(s.fr + 6, w);
}

struct DofRows { float fl, fD, fR, faref, lims, laref, lD, jf, jl, pf, pl; };  // fR = 1/fD

__device__ __forceinline__ float cone_cost(const Slot& s) {
  float f[3], W[6];
  const float D[3] = {s.D0, s.D1, s.D1};
  return cone_eval(s.jar, D, s.Dm, s.mu, s.fri, f, W);
}

__device__ __forceinline__ float dof_rows_cost(const DofRows& dr) {
  float cs = 0.f;
  if (dr.fl > 0.f) {
    const float R = dr.fR, x = dr.jf, fl = dr.fl;
    if (x <= -R * fl) cs += -0.5f * R * fl * fl - fl * x;
    else if (x >= R * fl) cs += -0.5f * R * fl * fl + fl * x;
    else cs += 0.5f * dr.fD * x * x;
  }
  if (dr.lims != 0.f && dr.jl < 0.f) cs += 0.5f * dr.lD * dr.jl * dr.jl;
  return cs;
}

// slope and curvature of the lane's rows along the search direction at step al (line search)
// (`used`: bit k set iff some lane of the WAVE has a contact in slot k.  An empty slot is all zeros -- its cone test reads `top`, its terms are zero -- so a slot is evaluated
// by every lane or skipped by the whole wave: no exec-masked region inside the line search's loop.)
template <int NS>
__device__ __forceinline__ void lane_rows_dir(const Slot* sl, const DofRows& dr, float al, float* d1, float* d2, unsigned used) {
  float g1 = 0.f, g2 = 0.f;
#pragma unroll
  for (int k = 0; k < NS; k++) {
    if (k > 0 && !((used >> k) & 1u)) continue;
    const float* jp = sl[k].jp;
    const float jar[3] = {fmaf(al, jp[0], sl[k].jar[0]), fmaf(al, jp[1], sl[k].jar[1]), fmaf(al, jp[2], sl[k].jar[2])};
    const float D[3] = {sl[k].D0, sl[k].D1, sl[k].D1};
    cone_dir(jar, jp, D, sl[k].Dm, sl[k].mu, sl[k].fri, &g1, &g2);
  }
  {  // the own dof's friction-loss and limit rows, as selects (the same fused multiply-adds as the branches they replace: same bits, a dozen exec-mask instructions fewer per evaluation)
    const float D = dr.fD, jp = dr.pf, x = fmaf(al, jp, dr.jf), fl = dr.fl, lim = dr.fR * fl;
    const bool has = fl > 0.f, lo_ = x <= -lim, hi_ = x >= lim, mid = has & !lo_ & !hi_;
    const float t = lo_ ? -fl : (hi_ ? fl : D * x);
    g1 = has ? fmaf(t, jp, g1) : g1;
    g2 = mid ? fmaf(D * jp, jp, g2) : g2;
    const float jl = dr.pl, xl_ = fmaf(al, jl, dr.jl);
    const bool lim_on = (dr.lims != 0.f) & (xl_ < 0.f);
    g1 = lim_on ? fmaf(dr.lD * xl_, jl, g1) : g1;
    g2 = lim_on ? fmaf(dr.lD * jl, jl, g2) : g2;
  }
  *d1 = g1; *d2 = g2;
}

// element j (run-time, wave-nonuniform) of a 4-array held in registers: compare-and-select
__device__ __forceinline__ float sel4(const float* a, int j) { return j == 0 ? a[0] : (j == 1 ? a[1] : (j == 2 ? a[2] : a[3])); }

// the same as two levels of selects with opaque results: the compiler cannot turn the chain into a branch on j and copy what follows into both sides (a quad holds all four j:
// it would run every copy)
__device__ __forceinline__ float sel4o(const float* a, int j) {
  float lo = (j & 1) ? a[1] : a[0], hi = (j & 1) ? a[3] : a[2];
  asm volatile("" : "+v"(lo), "+v"(hi));
  float r = (j & 2) ? hi : lo;
  asm volatile("" : "+v"(r));
  return r;
}

// Elimination order of the four finger chains when contacts couple them (hand self-collision).  `cmask` has bit 4a + b for every coupled pair a < b.
// A coupling graph without a cycle is eliminated leaf first: every chain is eliminated when at most one of its neighbours is left (its parent, which
// receives the Schur update); `level` is the stage at which chain c goes, `maxlev` the last stage of the rollout.  Returns false for a graph with a
// cycle (elimination would create a block between two chains that had none): those rollouts take the dense direction.
__device__ __forceinline__ int pidx(int a, int b) { return a * (7 - a) / 2 + (b - a - 1); }  // index of the chain pair a < b: 01 02 03 12 13 23
__device__ __forceinline__ bool chain_elim_order(int cmask, int c, int& level, int& parent, int& maxlev) {
  int adj[NCH] = {0, 0, 0, 0};
#pragma unroll
  for (int a = 0; a < NCH; a++)
#pragma unroll
    for (int b = a + 1; b < NCH; b++) if ((cmask >> (4 * a + b)) & 1) { adj[a] |= 1 << b; adj[b] |= 1 << a; }
  int rem = 0xF; bool ok = true;
  level = 0; parent = -1; maxlev = 0;
#pragma unroll
  for (int st = 0; st < NCH; st++) {
    int elig = 0, pr[NCH] = {-1, -1, -1, -1};
#pragma unroll
    for (int a = 0; a < NCH; a++) if ((rem >> a) & 1) {
      const int nbm = adj[a] & rem, deg = __popc(nbm);
      if (deg == 0) elig |= 1 << a;
      else if (deg == 1) {
        const int nb = __ffs(nbm) - 1;
        const int anb = nb == 0 ? adj[0] : (nb == 1 ? adj[1] : (nb == 2 ? adj[2] : adj[3]));
        if (__popc(anb & rem) > 1 || a < nb) { elig |= 1 << a; pr[a] = nb; }
      }
    }
    if (rem != 0 && elig == 0) ok = false;
    if (elig != 0) maxlev = st;
#pragma unroll
    for (int a = 0; a < NCH; a++) if (((elig >> a) & 1) && a == c) { level = st; parent = pr[a]; }
    rem &= ~elig;
  }
  return ok;
}

// ------------------------------------------------------------------------------------------------ the kernel
// PERSIST (fused mode, launches with more groups of four rollouts than the GPU has wave slots): the launch has one workgroup per resident slot, and every wave runs a queue of
// groups -- first the one of its own global wave index, then tickets drawn from `head` (zeroed by the launcher in front of the kernel) with one returning device-scope
// atomicAdd by lane 0 -- until the tickets pass the group count.  A wave slot is then never held for a workgroup-mate's longer rollouts, and the launch drains over one
// group's duration per wave instead of one workgroup's.  No wave waits for another, so nothing depends on which workgroups are resident.  The static instantiations
// (PERSIST = false: a wave's group is its place in the grid, `head` unused) compile to the code they had without it.
// Horizon slices (`slices_` & 0xff = S > 1): a queue unit is (group, slice) -- ticket t in [0, S * groups) is slice t / groups of group t % groups, all first slices in front
// of all second ones, and slice s runs steps [s H / S, (s + 1) H / S) -- so that the launch drains over a slice's duration instead of a group's.  A slice that is not the
// last parks what the step loop carries (PARK_F floats per unit, rows of 64 lanes: q, qd, the joints' warm start, then per rollout the cube's state, the running cost and
// the cube's warm start) behind the flag words in `pflags`, fences at device scope and sets the unit's flag; the next slice's wave reads that flag ONCE.  Set: it fences
// and resumes from the parked rows (fp32 out, fp32 in).  Not set (the producer is still running; or bit 8 of `slices_`, a test hook): it runs the group from x0 up to its
// slice's first step (bit 9 of `slices_`: slice s runs steps [sb_[s - 1], sb_[s]) of the bounds table instead, S <= 16: slices that shorten towards the end of the horizon, so
// that the tickets drawn last are the short ones) -- the same instructions on the same inputs, the same bits; trace rows written twice carry the same words -- zeroes the counters and goes on into its own
// slice.  While it recomputes it adds to no counter (`stats` is null for that pass: the dropped contacts and lost candidate pairs of those steps are the producer's to count) and
// its contacts above the LDS pool go to a row of its wave slot's own behind the rollouts' rows (the producer may still be running the same rollouts on theirs); the
// launch counts such units in stats[JH_STAT_RECOMPUTED].  Nothing polls and no wave waits for another.  Every flag and every parked row is written by one unit and read by at most one, once per launch.
// BATCH (fused mode, static grid only -- there is NO queue for batched launches: a batch's problems fill the GPU side by side, and a queue across problems would have to
// re-stage a workgroup's task parameters per group): B independent problems in one launch (jh_plan_step_batch), grid (groups of a problem, B).  A workgroup stages sTp once,
// so it belongs to one problem, blockIdx.y; everything a problem owns -- its packed block (x0, nominal, sigma, task parameters, bounds: `batch_blk` floats apart), its noise
// (`batch_noise` floats apart), its costs, trace rows and overflow rows (N rollouts apart) -- is reached by offsetting the kernel's pointers once, at the top, with
// arithmetic on kernel arguments and blockIdx.y alone: the bases stay in SGPRs, and a rollout's code below is the single launch's.  A model set
// (jh_plan_step_batch_models) gives every problem its own image of the float section as well, `batch_image` floats apart (0: one image for all); the int section --
// topology, pair lists, lane lists -- is one for the launch.  The plant axis (jh_plan_step_randomized; jh_internal.h) makes the problems blocks of ONE problem's rollouts:
// a stride on the global rollout index, so that only global rollout 0 is the noise-free nominal, and a by-value table from the problem to its image in place of the
// problem's own index -- 0 and the identity for every other batched launch.  The other instantiations ignore the three strides and compile to the code they had without them.
// BATCH with MATERIALIZE (jh_rollout_materialize_plants): the blocks of a materialise launch, each on a plant of a model set -- the same grid and the same by-value table,
// the strides put to the block's controls, x0 and image (below, at the top of the kernel).
template <bool MATERIALIZE, int WPB, bool SELF, bool PERSIST = false, bool BATCH = false>
__global__ __launch_bounds__(WAVE * WPB, WAVES_PER_EU) void k_leap_v5(const float* __restrict__ gF, const int* __restrict__ gI, const float* __restrict__ x0, int x0_batched,
                                                   const float* __restrict__ nominal, const float* __restrict__ noise, int ldn,
                                                   const float* __restrict__ sigma, const float* __restrict__ W, const float* __restrict__ lohi,
                                                   const float* __restrict__ tp, int N, int n_offset, int H, int K, float* __restrict__ costs,
                                                   float* __restrict__ knots_out, const float* __restrict__ controls, float* __restrict__ states,
                                                   float* __restrict__ sensors, int* __restrict__ stats_, int dshift_, float* __restrict__ trace, float* __restrict__ ovf_all_, unsigned* __restrict__ head,
                                                   long long batch_blk, long long batch_noise, long long batch_image, unsigned* pflags, int slices_,
                                                   std::conditional_t<BATCH, BatchBounds, SliceBounds> sb_) {
  static_assert(!BATCH || !PERSIST, "batched launches run on the static grid");
  if constexpr (BATCH && MATERIALIZE) {
    // Materialise mode on a plant axis (jh_rollout_materialize_plants), grid (groups of a block, G): block blockIdx.y is N rollouts of its own on the image its table
    // entry names.  The three strides are the block's here -- `batch_blk` floats to the next block's controls (0: every block reads rows [0, N)), `batch_noise` to its
    // rows of x0 (0: one state for the launch), `batch_image` to the next image -- and its rows of states, sensors and overflow lie N rollouts behind the
    // block before.  Pointer offsets from kernel arguments and blockIdx.y alone; below, N is the block's and a rollout's code is the single launch's.
    const long long pb = blockIdx.y;
    gF += jh_plant_of(sb_.plants, (int)pb, (int)pb) * batch_image;
    x0 += pb * batch_noise; controls += pb * batch_blk;
    if (states) states += pb * N * H * NX;
    if (sensors) sensors += pb * N * H * gI[HI_NS];
    if (NOVF > 0 && ovf_all_) ovf_all_ += pb * N * (NOVF * POOL_F);
  }
  if constexpr (BATCH && !MATERIALIZE) {
    // blockIdx.z: the controller of jh_plan_step_ensemble_batch, whose M plants are the problems of blockIdx.y -- strides of its own in sb_ (all 0 and gridDim.z == 1 for
    // every other batched launch); `pr`: the (controller, problem) pair, which owns the costs, trace and overflow rows
    const long long pb = blockIdx.y, pc = blockIdx.z, pr = pc * gridDim.y + pb;
    const long long ob = pb * batch_blk + pc * axis_stride(sb_, 0);
    x0 += ob; nominal += ob; sigma += ob; lohi += ob; tp += ob;
    // the plant axis (jh_plan_step_randomized): the problem's first global rollout index and the image its table names -- 0 and image pb for every other launch; the
    // table's entry is the pair's, `pr` (jh_plan_step_randomized_batch: an assignment per controller), which is pb wherever gridDim.z == 1
    n_offset += (int)pb * sb_.plants.n_stride;
    noise += pb * batch_noise + pc * axis_stride(sb_, 1); costs += pr * N; gF += jh_plant_of(sb_.plants, (int)pr, (int)pb) * batch_image + pc * axis_stride(sb_, 2);
    if (trace) trace += pr * N * H * 15;
    if (NOVF > 0 && ovf_all_) ovf_all_ += pr * N * (NOVF * POOL_F);  // (the overflow rows are indexed by rollout: a problem's N rows behind the one before)
  }
  __shared__ RS sRS[RPW * WPB];
  __shared__ float sBody[16 * BFS];
  __shared__ float sTp[16];
  __shared__ float sGeomF[MAXG * GEOM_F];
  __shared__ int sGeomI[MAXG * GEOM_I];
  __shared__ int sLaneG[16 * MAXLG];
  __shared__ float sLane[16 * LC_N];
  __shared__ int sBP[SELF ? 2 * MAXBP : 4];    // hand body pairs (side A, side B): every geom of A is a candidate against every geom of B
  __shared__ int sBG[SELF ? 2 * NBC : 4];    // per hand body: first collision geom, number of geoms (contiguous in the geom table)
  __shared__ float sBB[SELF ? NBC * 8 : 4];  // per hand body: bounding-box centre (body frame; static geometry: world), bounding radius, half sizes
  __shared__ int sGrp[WPB];  // PERSIST: the group each wave is running (re-read in the step loop instead of held in a register; unused and dropped otherwise)
  __shared__ int sUnit[4 * WPB];  // PERSIST, per wave: the step at which the running pass of the step loop ends, the unit's first step, the step behind its last, its ticket (in LDS for the reason sGrp is)
  const int dshift = PERSIST ? 0 : dshift_;  // (the queue is for launches that fill the GPU: never the latency mode)
#ifdef JH_V5_WAVESTAMP  // diagnostic builds (tools/diag/wave_schedule.py): per group of four rollouts, the 100 MHz wall clock at the wave's entry, after the staging barrier, at the
                         // group's start and end, with the workgroup, the wave and the hardware id (__smid) that ran it
  const unsigned long long ws_entry = wall_clock64(); unsigned long long ws_staged = ws_entry;
#endif
  const int tid = threadIdx.x, wv = tid >> 6, lane = tid & 63, r = lane >> 4;
  int l = lane & 15, c = l >> 2, s = l & 3;  // (not const: see the top of the step loop)
  RS& S = sRS[wv * RPW + r];
  const int nmI = gI[HI_NM], nblkI = gI[HI_NBLK], nuI = gI[HI_NU], ngI = gI[HI_NG], nsiteI = gI[HI_NSITE], nsI = gI[HI_NS], oRef = gI[HI_REF];
  const int oBodyF = HEADER_F, oDofF = oBodyF + nmI * BODY_F, oActF = oDofF + gI[HI_NV] * DOF_F, oGeomF = oActF + nuI * ACT_F, oSiteF = oGeomF + ngI * GEOM_F;
  const int oGeomI = HEADER_I + nmI * BODY_I + nblkI * BLOCK_I + nuI * ACT_I, oSiteI = oGeomI + ngI * GEOM_I;
  const int oLane = gI[HI_LANES], lgm = gI[HI_LGM];
  const int oBP = gI[HI_BP], oBS = gI[HI_BS], nBP = gI[HI_NBP], oBG = oBP + 2 * nBP;  // hand self-collision: body pairs, body bounding volumes, per-body geom ranges
  for (int i = tid; i < 16 * BODY_F; i += WAVE * WPB) sBody[(i / BODY_F) * BFS + i % BODY_F] = gF[oBodyF + BODY_F + i];
  for (int i = tid; i < ngI * GEOM_F; i += WAVE * WPB) sGeomF[i] = gF[oGeomF + i];
  for (int i = tid; i < ngI * GEOM_I; i += WAVE * WPB) sGeomI[i] = gI[oGeomI + i];
  for (int i = tid; i < 16 * lgm; i += WAVE * WPB) sLaneG[i] = gI[oLane + i];
  if (!MATERIALIZE && tid < 9) sTp[tid] = tp[tid];
  if constexpr (SELF) {
    for (int i = tid; i < 2 * nBP && i < 2 * MAXBP; i += WAVE * WPB) sBP[i] = gI[oBP + i];
    for (int i = tid; i < 2 * NBC; i += WAVE * WPB) sBG[i] = gI[oBG + i];
    for (int i = tid; i < NBC * 8; i += WAVE * WPB) sBB[i] = gF[oBS + i];
  }
  if (tid < 16) {
    const float* df = gF + oDofF + (6 + l) * DOF_F; const float* af = gF + oActF + l * ACT_F;
    float* lc = sLane + l * LC_N;
    lc[LC_DAMP] = df[DF_DAMP]; lc[LC_KVD] = df[DF_KV]; lc[LC_FL] = df[DF_FL]; lc[LC_FB] = df[DF_FB]; lc[LC_FD] = df[DF_FD]; lc[LC_INVW] = df[DF_INVW];
    lc[LC_LIMITED] = df[DF_LIMITED]; lc[LC_LO] = df[DF_LO]; lc[LC_HI] = df[DF_HI]; lc[LC_LK] = df[DF_LK]; lc[LC_LB] = df[DF_LB];
    for (int k = 0; k < 5; k++) lc[LC_SI + k] = df[DF_SOLIMP + k];
    lc[LC_KP] = af[AF_KP]; lc[LC_KV] = af[AF_KV]; lc[LC_CLIM] = af[AF_CLIM]; lc[LC_CLO] = af[AF_CLO]; lc[LC_CHI] = af[AF_CHI];
    // (the convergence test's scale of the cube's dofs: read from here in every iteration -- kept in a register across the loop it is spilled to scratch memory)
    lc[LC_IMCK] = l < 6 ? 1.f / (l < 3 ? gF[HF_CMASS] : gF[HF_CINERTIA + (l < 3 ? 0 : l - 3)]) : 0.f;
  }
  const float* lc = sLane + l * LC_N;
  // Rollout handled by this row of 16 lanes.  A launch too small to fill the GPU (`dshift` > 0, chosen by the launcher) gives a wave 4 >> dshift rollouts instead of four and
  // lets 1 << dshift rows compute the same one: the copies run the same arithmetic (a rollout's result does not depend on its wave-mates), only the first writes, and the
  // wave no longer waits for the slowest of four different Newton solves in every step -- the latency mode of small shards and of the reference's 32-rollout configurations.
  int grp = blockIdx.x * WPB + wv;  // the group of 4 >> dshift rollouts this wave runs: static launches have one per wave, its place in the grid
  const int ngroups = (N + RPW - 1) / RPW;
  if constexpr (PERSIST) {
    __syncthreads();  // the only workgroup barrier: the model image is staged (once per workgroup, for all the groups its waves will run)
#ifdef JH_V5_WAVESTAMP
    ws_staged = wall_clock64();
#endif
  }
  int unit = grp;  // PERSIST: the ticket of the unit this wave runs
  const int nsl = PERSIST ? max(1, min(slices_ & 0xff, H)) : 1, nunits = nsl * ngroups;
  float* park = (float*)(pflags + ((nunits + 3) & ~3));  // (PERSIST, nsl > 1; never read through a const or __restrict__ pointer: other waves write it during the launch)
  bool again = false;  // PERSIST: the unit's hand-off was missed and the steps in front of its slice have been recomputed: the next pass of the loop below runs the slice itself
  float q, qd, qc[7], vc[6], acc;  // the state the step loop carries: own joint, the replicated cube, the running cost (declared here: kept from the one pass to the other)
#ifdef JH_V5_WAVESTAMP
  unsigned long long ws_start = 0;
#endif
  for (; !PERSIST || unit < nunits;) {  // one pass for a static launch (it leaves at the bottom); the queue's units otherwise.  (The body keeps the kernel's indentation.)
  bool resumed = false, prefix = false; int hh0 = 0;  // PERSIST: the previous slice's state was parked in time / was not, and this pass recomputes the steps in front of the slice; the step this pass starts at (0: the group's start, also for a slice whose hand-off was missed)
  if constexpr (PERSIST) if (again) {  // (the state is in registers and in S.ws; the counters below start from zero: the recomputed steps are another unit's to count)
    unit = __builtin_amdgcn_readfirstlane(sUnit[4 * wv + 3]); grp = unit % ngroups; hh0 = __builtin_amdgcn_readfirstlane(sUnit[4 * wv + 1]);
    const int h1 = __builtin_amdgcn_readfirstlane(sUnit[4 * wv + 2]);
    WSYNC();
    if (lane == 0) sUnit[4 * wv] = h1;
  }
  if constexpr (PERSIST) if (!again) {
    grp = unit % ngroups;
    const int sl = unit / ngroups; int h0 = sl * H / nsl, h1 = (sl + 1) * H / nsl;
    if (slices_ & 0x200) {  // slices of unequal length: the table of bounds (at most 16 slices), read here and nowhere else -- h0 and h1 go into the unit's words below as ever
      const auto bound = [&](int i) -> int { return (int)((sb_.w[i >> 1] >> ((i & 1) << 4)) & 0xffffu); };
      h1 = bound(sl); h0 = sl > 0 ? bound(sl - 1) : 0;
    }
    if (sl > 0) {  // the flag of (group, slice - 1), read once: an acquire load of lane 0, broadcast, and the wave's acquire fence in front of the parked rows
      unsigned f = 0;
      if (lane == 0 && !(slices_ & 0x100)) f = __hip_atomic_load(pflags + (unit - ngroups), __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT);
      resumed = __builtin_amdgcn_readfirstlane(f) != 0;
      if (resumed) { __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent"); hh0 = h0; }
      prefix = !resumed;
    }
    if (lane == 0) { sGrp[wv] = grp; sUnit[4 * wv] = (sl == 0 || resumed) ? h1 : h0; sUnit[4 * wv + 1] = h0; sUnit[4 * wv + 2] = h1; sUnit[4 * wv + 3] = unit; }  // (published to the wave by the WSYNC in front of the step loop)
  }
#ifdef JH_V5_WAVESTAMP
  if (!PERSIST || !again) ws_start = wall_clock64();
#endif
  const int n = (grp << (2 - dshift)) + (r >> dshift);
  const bool live = n < N && (r & ((1 << dshift) - 1)) == 0;
  const int nc = n < N ? n : N - 1;
  // What the pass counts into and where its contacts above the LDS pool go: the launch's counters and the rollout's overflow row -- except while a missed hand-off is
  // recomputed (PERSIST): nothing is counted, and the row is one of this wave slot's own, behind the N rollouts' (the code below indexes by the rollout: hence the offset).
  int* stats = stats_; float* ovf_all = ovf_all_;
  if constexpr (PERSIST) if (prefix) {
    stats = nullptr;
    if (NOVF > 0 && ovf_all_) ovf_all = ovf_all_ + ((long long)N + (long long)(blockIdx.x * WPB + wv) * RPW + r - nc) * (NOVF * POOL_F);
  }
  const float h = gF[HF_DT], impratio = gF[HF_IMPRATIO], tol = gF[HF_TOL], lstol = gF[HF_LSTOL]; const int cap = (int)gF[HF_MAXITER];
  const float grav[3] = {gF[HF_GRAV], gF[HF_GRAV + 1], gF[HF_GRAV + 2]};
  const float cmass = gF[HF_CMASS], cI[3] = {gF[HF_CINERTIA], gF[HF_CINERTIA + 1], gF[HF_CINERTIA + 2]};
  const float chs[3] = {gF[HF_CSIZE], gF[HF_CSIZE + 1], gF[HF_CSIZE + 2]}, crb = gF[HF_CRBOUND], ctran = gF[HF_CTRAN];
  const float cK = gF[HF_CK], cB = gF[HF_CB];
  float csi[5]; for (int k = 0; k < 5; k++) csi[k] = gF[HF_SOLIMP + k];
  // own cube dof (lanes 0..5): inertia and its inverse; zero elsewhere
  const float mck = (l < 3 ? cmass : (l == 3 ? cI[0] : (l == 4 ? cI[1] : (l == 5 ? cI[2] : 0.f))));
  // ---- state: own joint + replicated cube
  if (!PERSIST || !again) {
    const float* xi = x0 + ((MATERIALIZE && x0_batched) ? (size_t)nc * NX : 0);
    for (int k = 0; k < 7; k++) qc[k] = xi[k];
    for (int k = 0; k < 6; k++) vc[k] = xi[NQ + k];
    q = xi[7 + l]; qd = xi[NQ + 6 + l];
  }
  // ---- own actuator's spline knots (fused mode): clip(nominal + sigma*noise) -> LDS; global sample 0 keeps the nominal
  // The knots are NOT kept on chip: 8 knots x 16 actuators are 512 B of LDS per rollout (a sixth of its state), and the step loop needs them once per step -- K
  // L2-resident loads of the noise matrix and of the nominal, issued ahead of the kinematics (`knot_at` below); the LDS goes to the contact pool instead.
  auto knot_at = [&](int k, int ll, int ncc) -> float {  // clip(nominal + sigma * noise) of actuator ll, knot k, rollout ncc (global sample 0 keeps the nominal)
    const int i = k * NU + ll;
    float v = nominal[i];
    if (n_offset + ncc != 0) v = fmaf(sigma[i], noise[(size_t)i * ldn + ncc], v);
    return jh_clampf(v, lohi[ll], lohi[NU + ll]);
  };
  if (!MATERIALIZE) {
    if (knots_out && live && (!PERSIST || unit < ngroups)) for (int k = 0; k < K; k++) knots_out[(size_t)(k * NU + l) * ldn + n] = knot_at(k, l, nc);
  }
  if (!PERSIST || !again) { S.ws[6 + l] = 0.f; if (l < 6) S.ws[l] = 0.f; }
  if (l < 4) S.cmd[l] = l == 0 ? cmass : (l == 1 ? cI[0] : (l == 2 ? cI[1] : cI[2]));
  int n_iters = 0, n_maxed = 0, n_wave_iters = 0;  // (the last: iterations this wave ran -- per step the maximum over its four rollouts)
  if (!PERSIST || !again) acc = 0.f;
  if constexpr (PERSIST) if (resumed) {  // the parked rows of (group, slice - 1): device-scope loads, one per lane and value
    float* pk = park + (size_t)(unit - ngroups) * PARK_F; const int r16 = lane & 48;
    q = PARK_LD(pk + lane); qd = PARK_LD(pk + 64 + lane); S.ws[6 + l] = PARK_LD(pk + 128 + lane);
    for (int k = 0; k < 7; k++) qc[k] = PARK_LD(pk + 192 + r16 + k);
    for (int k = 0; k < 6; k++) vc[k] = PARK_LD(pk + 199 + r16 + k);
    acc = PARK_LD(pk + 205 + r16);
    if (l < 6) S.ws[l] = PARK_LD(pk + 256 + lane);
  }
#ifdef JH_V5_TICKS  // shader-clock totals per phase (diagnostic builds; tools/diag/profile_v5.py): 0 kinematics+dynamics, 1 broad phase, 2 narrow phase, 3 rows+warm start,
                     // 4 gradient, 5 Newton matrix, 6 factorisation+direction, 7 line search+step and integration
  long long cyc[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, t0 = clock64();
#define V5_TICK(slot) { long long t__ = clock64(); cyc[slot] += t__ - t0; t0 = t__; }
  // finer split (tools/diag/profile_v5b.py reads stats[384..]): 8 convergence test + Hessian initialisation, 9 Schur complement + 6x6 + back-substitution (the rest of 6 is the chain
  // blocks), 10 line-search set-up (M p, J p), 11 the slope evaluations, 12 step
#else
#define V5_TICK(slot)
#endif
#ifdef JH_V5_COUNT
  int cnt_dense = 0, cnt_it = 0, cnt_l2 = 0, cnt_bp = 0, cnt_hh = 0, cnt_cls[4] = {0, 0, 0, 0};
  // the broad phase's lane use (tools/diag/count_broadphase.py; profiles/leap_broad_phase.md), stats[34..55].  Sums over rollout-steps (R) or wave-steps (W), maxima (M):
  // 34 R sphere survivors of level 1, 35 W their maximum over the wave, 36 W the maximum of the box survivors, 37 W passes of 16 body pairs with a sphere survivor (= runs of the
  // box region in the per-pair form), 38 W ceil(35 / 16) (= runs in the list form), 39 W trips of a loop over the near geoms of side A in level 2 (b) (the form before the combination passes: stays zero), 40 R body pairs that reach (b), 41 R their
  // combinations T = near A x near B, 42 W passes of 16 combinations, 43 W geom slots of the cube's sweep with a lane in the box region, 44 lanes in it, 45 M sphere survivors,
  // 46 M box survivors, 47 M T, 48 R steps without a sphere survivor, 49 / 50 R pairs in (b) with one near geom on side A / B, 51 R trips a rollout needs by itself,
  // 52 R steps with more than MAXBPL sphere survivors, 53 M MAXBP - sphere survivors (the fewest seen)
  enum { CB_SPH = 34, CB_SPHMAX, CB_BOXMAX, CB_L1PAIRPASS, CB_L1LISTPASS, CB_TRIPS, CB_BPAIRS, CB_T, CB_COMBOPASS, CB_CUBEBOX, CB_CUBEBOXLANES, CB_MSPH, CB_MBOX, CB_MT, CB_NOSPH, CB_ONEA, CB_ONEB,
         CB_OWNTRIPS, CB_SPHOVER, CB_FEWSPH, CB_TSAFE, CB_TDROP };  // 54 R pairs whose table reads safe, 55 R those of them with overlapping bounding spheres (dropped from the list)
#define V5_CADD(k, v) do { if (stats) atomicAdd(stats + (k), (int)(v)); } while (0)
#define V5_CMAX(k, v) do { if (stats) atomicMax(stats + (k), (int)(v)); } while (0)
#endif
  if constexpr (PERSIST) WSYNC();  // (this group's S.ws / S.cmd / sGrp; the workgroup barrier was taken once, in front of the queue)
  else {
    __syncthreads();  // the only workgroup barrier: the model image is staged
#ifdef JH_V5_WAVESTAMP
    ws_staged = wall_clock64();
#endif
  }

  const int hend = PERSIST ? __builtin_amdgcn_readfirstlane(sUnit[4 * wv]) : H;  // (a scalar register across the loop: re-read from LDS at every step it cost the loop 30 spilled VGPRs)
  for (int hh = hh0; hh < hend; hh++) {
    // the model constants of a lane (sBody, sLane, ...) do not change over the steps: left alone the compiler loads them once before the loop, runs out of
    // registers and reloads them from scratch memory in every step instead of from LDS
    OPAQUE(l); c = l >> 2; s = l & 3;
    const float* lc = sLane + l * LC_N;
    // ================================================================ controls
    float u;
    if (MATERIALIZE) u = controls[((size_t)nc * H + hh) * NU + l];
    else {
      u = 0.f;
      {  // (the rollout index is recomputed from an opaque copy of the lane id: held across the step loop it would cost a register the loop does not have)
        int lo_ = lane; OPAQUE(lo_);
        const int g_ = PERSIST ? sGrp[wv] : (int)(blockIdx.x * WPB + wv);
        const int n_ = (g_ << (2 - dshift)) + ((lo_ >> 4) >> dshift), nc_ = n_ < N ? n_ : N - 1;
        for (int k = 0; k < K; k++) u = fmaf(W[hh * K + k], knot_at(k, l, nc_), u);
      }
    }
    // ================================================================ kinematics (each lane walks its chain up to its own link)
    float Mrow[NLK], fs_own, a0_own;
    {
      float ax[NLK][3], og[NLK][3], Rown[9], pown[3];
      {
        float nn = rsqrtf(qc[3] * qc[3] + qc[4] * qc[4] + qc[5] * qc[5] + qc[6] * qc[6]);
        qc[3] *= nn; qc[4] *= nn; qc[5] *= nn; qc[6] *= nn;
        float Rc[9]; quat2mat(Rc, qc + 3);
        float P[3] = {0, 0, 0}, R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
        float sn_own, cs_own; sincosf(q, &sn_own, &cs_own);
#pragma unroll
        for (int j = 0; j < NLK; j++) {
          const float* bf = sBody + (4 * c + j) * BFS;
          float P2[3], R0[9];
          if (j == 0) { for (int k = 0; k < 3; k++) P2[k] = bf[BF_LPOS + k]; for (int k = 0; k < 9; k++) R0[k] = bf[BF_LR + k]; }
          else { mulMV(P2, R, bf + BF_LPOS); for (int k = 0; k < 3; k++) P2[k] += P[k]; mulMM(R0, R, bf + BF_LR); }
          const float* al = bf + BF_AXIS;
          mulMV(ax[j], R0, al);
          for (int k = 0; k < 3; k++) { og[j][k] = P2[k]; P[k] = P2[k]; }
          const float sn = quad_get(sn_own, j), cs = quad_get(cs_own, j), t = 1.f - cs, x = al[0], y = al[1], z = al[2];
          float Rq[9] = {t * x * x + cs, t * x * y - sn * z, t * x * z + sn * y, t * x * y + sn * z, t * y * y + cs, t * y * z - sn * x, t * x * z - sn * y, t * y * z + sn * x, t * z * z + cs};
          mulMM(R, R0, Rq);
          if (j == s) { for (int k = 0; k < 3; k++) pown[k] = P2[k]; for (int k = 0; k < 9; k++) Rown[k] = R[k]; }
        }
        for (int k = 0; k < 3; k++) { S.pa[1 + l][k] = pown[k]; S.pa[1 + l][4 + k] = s == 0 ? ax[0][k] : (s == 1 ? ax[1][k] : (s == 2 ? ax[2][k] : ax[3][k])); }
        for (int k = 0; k < 9; k++) S.xR[1 + l][k] = Rown[k];
        if (l == 0) { for (int k = 0; k < 3; k++) S.pa[0][k] = qc[k]; for (int k = 0; k < 9; k++) S.xR[0][k] = Rc[k]; S.ncon = 0; S.nhit = 0; }
        S.qv[6 + l] = qd;
        if (l < 6) S.qv[l] = vc[l];
      }
      // fused mode with a trace buffer (jh_rollout_cost_traced): the five trace sites of this forward pass -- what the materialise mode writes as sensors 16..30 --
      // for EVERY rollout: 60 B per rollout-step, 250 MB per plan step of the headline workload, and `Controller.traces` becomes a gather instead of a re-rollout
      if (!MATERIALIZE && trace && nsI == NS) {
        WSYNC();
        if (live && l < nsiteI && l < 5) {
          int b = gI[oSiteI + l]; float p3[3]; mulMV(p3, S.xR[b], gF + oSiteF + l * SITE_F);
          float* tr = trace + ((size_t)n * H + hh) * 15 + 3 * l;
          for (int k = 0; k < 3; k++) tr[k] = p3[k] + S.pa[b][k];
        }
      }
      // sensors of this forward pass (materialise mode): 16 joint positions, then 5 site positions
      if (MATERIALIZE && sensors) {
        float* y = sensors + ((size_t)nc * H + hh) * nsI;
        if (live) y[l] = q;
        WSYNC();
        if (nsI == NS) {  // leap_cube / leap_cube_down: five site positions
          if (live && l < nsiteI && l < 5) {
            int b = gI[oSiteI + l]; float p3[3]; mulMV(p3, S.xR[b], gF + oSiteF + l * SITE_F);
            for (int k = 0; k < 3; k++) y[16 + 3 * l + k] = p3[k] + S.pa[b][k];
          }
        } else if (live && l < 7) {  // caltech_leap_cube: cube position in the (world-fixed) grasp-site frame, cube orientation relative to the goal body's
          const float* rf = gF + oRef;  // [p_ref(3), R_ref(9), q_ref(4)]
          if (l < 3) y[16 + l] = rf[3 + l] * (qc[0] - rf[0]) + rf[6 + l] * (qc[1] - rf[1]) + rf[9 + l] * (qc[2] - rf[2]);
          else {
            const float a0 = rf[12], a1 = -rf[13], a2 = -rf[14], a3 = -rf[15], b0 = qc[3], b1 = qc[4], b2 = qc[5], b3 = qc[6];  // conj(q_ref) * q_cube
            const float qo[4] = {a0 * b0 - a1 * b1 - a2 * b2 - a3 * b3, a0 * b1 + a1 * b0 + a2 * b3 - a3 * b2, a0 * b2 - a1 * b3 + a2 * b0 + a3 * b1, a0 * b3 + a1 * b2 - a2 * b1 + a3 * b0};
            y[16 + l] = l == 3 ? qo[0] : (l == 4 ? qo[1] : (l == 5 ? qo[2] : qo[3]));
          }
        }
      }
      // ================================================================ chain dynamics: inertia block, bias, smooth force
      {
        const float* bf = sBody + (4 * c + s) * BFS;
        float Rk[9], rr[3], cs3[3]; mulMM(Rk, Rown, bf + BF_IR); mulMV(rr, Rown, bf + BF_IPOS);
        for (int k = 0; k < 3; k++) cs3[k] = pown[k] + rr[k];
        const float mass = bf[BF_MASS]; const float* di = bf + BF_INERTIA;
        float wv[3] = {0, 0, 0}, al[3] = {0, 0, 0}, ao[3] = {-grav[0], -grav[1], -grav[2]};
#pragma unroll
        for (int j = 0; j < NLK; j++) {
          float qdj = quad_get(qd, j);
          if (j <= s) {
            if (j > 0) {
              float d[3] = {og[j][0] - og[j - 1][0], og[j][1] - og[j - 1][1], og[j][2] - og[j - 1][2]}, t1[3], t2[3], t3[3];
              cross3(t1, wv, d); cross3(t2, wv, t1); cross3(t3, al, d);
              for (int k = 0; k < 3; k++) ao[k] += t3[k] + t2[k];
            }
            float wxa[3]; cross3(wxa, wv, ax[j]);
            for (int k = 0; k < 3; k++) { al[k] += wxa[k] * qdj; wv[k] += ax[j][k] * qdj; }
          }
        }
        float t1[3], t2[3], t3[3], ac3[3];
        cross3(t1, wv, rr); cross3(t2, wv, t1); cross3(t3, al, rr);
        for (int k = 0; k < 3; k++) ac3[k] = ao[k] + t3[k] + t2[k];
        float Iw[3], Ia[3], gy[3]; inertia_mul(Iw, Rk, di, wv); inertia_mul(Ia, Rk, di, al); cross3(gy, wv, Iw);
        float Fk[3] = {mass * ac3[0], mass * ac3[1], mass * ac3[2]}, Nk[3] = {Ia[0] + gy[0], Ia[1] + gy[1], Ia[2] + gy[2]};
        float bias[NLK], Mc[10];
        for (int k = 0; k < 10; k++) Mc[k] = 0.f;
#pragma unroll
        for (int i = 0; i < NLK; i++) {
          bias[i] = 0.f;
          if (i <= s) {
            float ri[3] = {cs3[0] - og[i][0], cs3[1] - og[i][1], cs3[2] - og[i][2]}, rxF[3], Jvi[3], tB[3];
            cross3(rxF, ri, Fk);
            bias[i] = ax[i][0] * (Nk[0] + rxF[0]) + ax[i][1] * (Nk[1] + rxF[1]) + ax[i][2] * (Nk[2] + rxF[2]);
            cross3(Jvi, ax[i], ri); inertia_mul(tB, Rk, di, ax[i]);
#pragma unroll
            for (int j = 0; j <= i; j++) {
              float rj[3] = {cs3[0] - og[j][0], cs3[1] - og[j][1], cs3[2] - og[j][2]}, Jvj[3]; cross3(Jvj, ax[j], rj);
              Mc[tri(i, j)] = mass * dot3(Jvi, Jvj) + dot3(tB, ax[j]);
            }
          }
        }
        for (int k = 0; k < 10; k++) Mc[k] = csum(Mc[k]);
        float bown = 0.f;
#pragma unroll
        for (int i = 0; i < NLK; i++) { float b = csum(bias[i]); if (i == s) bown = b; }
        // position servo on the own joint
        float cc = u; if (lc[LC_CLIM] != 0.f) cc = jh_clampf(cc, lc[LC_CLO], lc[LC_CHI]);
        fs_own = -lc[LC_DAMP] * qd - bown + lc[LC_KP] * (cc - q) - lc[LC_KV] * qd;
        float x4[4], L[10];
#pragma unroll
        for (int j = 0; j < NLK; j++) x4[j] = quad_get(fs_own, j);
        for (int k = 0; k < 10; k++) L[k] = Mc[k];
        float inv4[4]; chol4(L, inv4); fwd4(L, inv4, x4); bwd4(L, inv4, x4);
        a0_own = sel4(x4, s);
#pragma unroll
        for (int j = 0; j < NLK; j++) { float v = 0.f;
#pragma unroll
          for (int i = 0; i < NLK; i++) if (i == s) v = Mc[i >= j ? tri(i, j) : tri(j, i)];
          Mrow[j] = v; }
        if (s == 0) for (int k = 0; k < 10; k++) S.Mbb[c][k] = Mc[k];
      }
    }
    // free cube: M = diag(m,m,m,I); own component of the unconstrained acceleration (lanes 0..5)
    float a0c_own = 0.f;
    {
      float Icw[3] = {cI[0] * vc[3], cI[1] * vc[4], cI[2] * vc[5]}, gc[3]; cross3(gc, vc + 3, Icw);
      (void)gc;  // isotropic inertia (model_is_leap): w x (I w) = 0 exactly -- the body-frame expression only carries its own rounding noise
      a0c_own = l < 3 ? (l == 0 ? grav[0] : (l == 1 ? grav[1] : grav[2])) : 0.f;
    }
    WSYNC();
    V5_TICK(0)
    // ================================================================ collision: broad phase (cube vs the lane's geoms; hand body pairs), balanced narrow phase
    bool hand_hits = false;  // this rollout has candidate geom pairs of the hand against itself or the static geometry this step (a superset of its contacts off the cube)
    {
      int nh = 0;
      float Rc[9]; for (int k = 0; k < 9; k++) Rc[k] = S.xR[0][k];
      const float* pw = S.pa[1 + l]; const float* Rw = S.xR[1 + l];
      if constexpr (SELF) {  // bounding volume of the own link for the hand's self-collision
        const float* b8 = sBB + 8 * (1 + l); float cw[3]; mulMV(cw, Rw, b8);
        S.bs[1 + l][0] = cw[0] + pw[0]; S.bs[1 + l][1] = cw[1] + pw[1]; S.bs[1 + l][2] = cw[2] + pw[2]; S.bs[1 + l][3] = b8[3];
        if (l < 4) { S.bs[0][l] = sBB[l]; for (int b = NMB; b < NBC; b++) S.bs[b][l] = sBB[8 * b + l]; }
      }
      // (round 6: shaped for latency, the same tests.  The loop was a chain of eight dependent LDS round trips per geom -- its id, its body, its position, ... each
      // behind the test before it -- and nine exec-masked regions.  Now: the lane's geom ids in one batch of loads, a geom's record in one more, the sphere test and the
      // cube-frame box test as straight-line code, one region for the geom's own box.)
      float pwr[3], Rwr[9];
      for (int k = 0; k < 3; k++) pwr[k] = pw[k];
      for (int k = 0; k < 9; k++) Rwr[k] = Rw[k];
      int gids[MAXLG];
#pragma unroll
      for (int i = 0; i < MAXLG; i++) gids[i] = i < lgm ? sLaneG[l * lgm + i] : -1;
#pragma unroll
      for (int i = 0; i < MAXLG; i++) {
        if (i >= lgm) break;
        const int gid = gids[i], g0 = gid < 0 ? 0 : gid;
        const float* gf = sGeomF + g0 * GEOM_F;
        const int gbody = sGeomI[g0 * GEOM_I], gtype = sGeomI[g0 * GEOM_I + 1];
        const float lp[3] = {gf[GF_POS], gf[GF_POS + 1], gf[GF_POS + 2]}, rb = gf[GF_RBOUND];
        float gp[3]; mulMV(gp, Rwr, lp); gp[0] += pwr[0]; gp[1] += pwr[1]; gp[2] += pwr[2];
        if (gbody < 0) { gp[0] = lp[0]; gp[1] = lp[1]; gp[2] = lp[2]; }
        const float dc[3] = {gp[0] - qc[0], gp[1] - qc[1], gp[2] - qc[2]}, rs = rb + crb;
        float cl[3]; mulMTV(cl, Rc, dc);
        bool hit = (gid >= 0) & (dot3(dc, dc) <= rs * rs) & (fabsf(cl[0]) <= chs[0] + rb) & (fabsf(cl[1]) <= chs[1] + rb) & (fabsf(cl[2]) <= chs[2] + rb);
#if JH_V5_CYL
        if (hit && gtype != GSPHERE) {  // (a cylinder's box in its own frame: (r, r, L))
          const bool cyl = gtype == GCYL;
          const float gh[3] = {gf[GF_SIZE], cyl ? gf[GF_SIZE] : gf[GF_SIZE + 1], cyl ? gf[GF_SIZE + 1] : gf[GF_SIZE + 2]};
          float gR[9], gl[3];
          if (gbody < 0) { for (int k = 0; k < 9; k++) gR[k] = gf[GF_R + k]; } else mulMM(gR, Rwr, gf + GF_R);
          mulMTV(gl, gR, dc);
          hit = fabsf(gl[0]) <= gh[0] + crb && fabsf(gl[1]) <= gh[1] + crb && fabsf(gl[2]) <= gh[2] + crb;
        }
#else
#ifdef JH_V5_COUNT
        if constexpr (SELF) { const unsigned long long bx = __ballot(hit && gtype == GBOX); if (lane == 0 && bx != 0) { V5_CADD(CB_CUBEBOX, 1); V5_CADD(CB_CUBEBOXLANES, __popcll(bx)); } }
#endif
        if (hit && gtype == GBOX) {
          float gR[9], gl[3];
          if (gbody < 0) { for (int k = 0; k < 9; k++) gR[k] = gf[GF_R + k]; } else mulMM(gR, Rwr, gf + GF_R);
          mulMTV(gl, gR, dc);
          hit = fabsf(gl[0]) <= gf[GF_SIZE] + crb && fabsf(gl[1]) <= gf[GF_SIZE + 1] + crb && fabsf(gl[2]) <= gf[GF_SIZE + 2] + crb;
        }
#endif
        unsigned m16 = (unsigned)((__ballot(hit) >> (16 * r)) & 0xFFFFull);
        int pos = nh + __popc(m16 & ((1u << l) - 1u));
        if (hit && pos < MAXHIT) S.hits[pos] = (unsigned short)gid;
        nh += __popc(m16);
      }
      WSYNC();
      V5_TICK(13)  // (fine split of the broad phase: 13 = the cube against the lane's geoms, 14 = hand body pairs, 1 = geom level of the surviving pairs)
      if constexpr (SELF) {
      // hand self-collision, level 1: body pairs whose bounding spheres overlap (106 candidate pairs after MuJoCo's static filters, 16 per pass)
      int nbl = 0;
      {
        // (round 6: shaped for latency, the same tests in the same order.  Per pass of 16 pairs the loop was three dependent LDS round trips -- the pair, its two spheres, the
        // boxes' poses -- times seven passes.  Now: every pass's pair in one batch of loads, every pass's sphere test in a second, then the box test of the passes that
        // have a survivor.)
        constexpr int NPASS = MAXBP / G;
        int pab[NPASS]; unsigned sph = 0;
#pragma unroll
        for (int i = 0; i < NPASS; i++) { const int pi = i * G + l, pj = pi < nBP ? pi : 0; pab[i] = sBP[2 * pj] | sBP[2 * pj + 1] << 8; }
#pragma unroll
        for (int i = 0; i < NPASS; i++) {
          const float* sa = S.bs[pab[i] & 0xFF]; const float* sb = S.bs[pab[i] >> 8];
          const float d[3] = {sa[0] - sb[0], sa[1] - sb[1], sa[2] - sb[2]}, rs = sa[3] + sb[3];
          sph |= ((i * G + l < nBP) & (dot3(d, d) <= rs * rs)) ? 1u << i : 0u;
        }
#ifdef JH_V5_COUNT
        {
          int ns = 0, npass = 0;
          for (int i = 0; i < NPASS; i++) { const unsigned long long b = __ballot((sph >> i) & 1u); ns += __popc((unsigned)((b >> (16 * r)) & 0xFFFFull)); npass += b != 0; }
          const int nsm = wave_rowmax(ns);
          if (l == 0 && live) { V5_CADD(CB_SPH, ns); V5_CMAX(CB_MSPH, ns); V5_CADD(CB_NOSPH, ns == 0); V5_CADD(CB_SPHOVER, ns > MAXBPL); V5_CMAX(CB_FEWSPH, MAXBP - ns); }
          if (lane == 0) { V5_CADD(CB_SPHMAX, nsm); V5_CADD(CB_L1PAIRPASS, npass); V5_CADD(CB_L1LISTPASS, (nsm + G - 1) / G); }
        }
#endif
        // pair tables (engine_model.py::hand_pair_tables): a body pair whose relative pose is a function of two joint angles carries an 8 x 8 bit grid over them, a set
        // bit = no pose in the cell gives the pair a level-2 candidate.  Such a pair is taken out here, behind the sphere test and in front of its box test: it would have gone through level 2 and
        // appended nothing, so S.hits[] keeps its entries and their order.  The angles are this step's `q` of the two joints' lanes -- what the kinematics above ran on --
        // taken per row of 16 lanes (a wave's rollouts differ); an angle off the grid, or a NaN, reads as unsafe.  The records are wave-uniform: scalar loads.
        // The header slot is read here, in every step, through an index the compiler cannot see through: held across the step loop it costs a register the loop does not have.
        // Records beyond the image's count are zero and rule nothing out (a zero word), so the loop runs over all PT_MAX without reading the count.
        int pt_slot = HI_PT; asm volatile("" : "+s"(pt_slot));
        const int oPT = gI[pt_slot];  // (0: an image without tables)
#pragma unroll 1
        for (int t = 0; oPT > 0 && t < PT_MAX; t++) {
          const int* T = gI + oPT + 1 + t * PT_I;
          // (the two angles of each of the wave's four rows through scalar registers, then the own row's by select: eight v_readlane and no vector temporaries --
          // two ds_bpermute cost the Newton loop three more scratch loads per iteration in the queue instantiation, profiles/leap_pair_tables.md section 3)
          const int qi = __float_as_int(q), ja = T[1], jb = T[2];
          const int a0 = __builtin_amdgcn_readlane(qi, ja), a1 = __builtin_amdgcn_readlane(qi, 16 + ja), a2 = __builtin_amdgcn_readlane(qi, 32 + ja), a3 = __builtin_amdgcn_readlane(qi, 48 + ja);
          const int b0 = __builtin_amdgcn_readlane(qi, jb), b1 = __builtin_amdgcn_readlane(qi, 16 + jb), b2 = __builtin_amdgcn_readlane(qi, 32 + jb), b3 = __builtin_amdgcn_readlane(qi, 48 + jb);
          const float qa = __int_as_float(r == 0 ? a0 : (r == 1 ? a1 : (r == 2 ? a2 : a3))), qb = __int_as_float(r == 0 ? b0 : (r == 1 ? b1 : (r == 2 ? b2 : b3)));
          const float fa = (qa - __int_as_float(T[3])) * __int_as_float(T[4]), fb = (qb - __int_as_float(T[5])) * __int_as_float(T[6]);
          const bool in = fa >= 0.f && fa < 8.f && fb >= 0.f && fb < 8.f;
          const unsigned long long w = (unsigned long long)(unsigned)T[7] | (unsigned long long)(unsigned)T[8] << 32;
          const bool safe = in && ((w >> (((int)fa + 8 * (int)fb) & 63)) & 1ull);
          const unsigned drop = (safe && l == (T[0] & (G - 1))) ? 1u << (T[0] / G) : 0u;  // (pair i * G + l is bit i of lane l)
#ifdef JH_V5_COUNT
          if (live && l == 0 && safe) V5_CADD(CB_TSAFE, 1);
          if (live && (sph & drop) != 0) V5_CADD(CB_TDROP, 1);  // (the one lane that holds the pair)
#endif
          sph &= ~drop;
        }
        // The candidate list S.hits[] of a rollout and step is the one a plain loop over the pairs would build, entry for entry and in the same order: the same tests on the
        // same operands, only on other lanes and in fewer, fuller passes (profiles/leap_broad_phase.md).  Level 1 is list-driven: the sphere survivors are written out in
        // ascending order, and the oriented-box test runs over that list 16 entries per pass instead of once per pass of 16 body pairs with a few lanes each.
        // the sphere survivors in ascending pair order -> S.bpl.  The list can hold every pair of the model (up to MAXBP), S.bpl MAXBPL of them: the tail goes to the contact
        // pool's storage, which nothing uses between the Newton solve of the last step and this step's narrow phase
        unsigned char* const tail = reinterpret_cast<unsigned char*>(&S.pool[0][0]);
        static_assert(sizeof(((RS*)nullptr)->pool) >= MAXBP - MAXBPL, "the tail of the sphere survivors fits the contact pool's storage");
        int nsl = 0;
#pragma unroll
        for (int i = 0; i < NPASS; i++) {
          if (i * G >= nBP) break;
          const bool hit = (sph >> i) & 1u;
          const unsigned m16 = (unsigned)((__ballot(hit) >> (16 * r)) & 0xFFFFull);
          const int pos = nsl + __popc(m16 & ((1u << l) - 1u));
          if (hit) { if (pos < MAXBPL) S.bpl[pos] = (unsigned char)(i * G + l); else tail[pos - MAXBPL] = (unsigned char)(i * G + l); }
          nsl += __popc(m16);
        }
        WSYNC();
        // the box test over the list, 16 entries per pass; the survivors go back to the front of S.bpl in the same order.  A pass reads its 16 entries before it writes
        // (the ballot needs every lane's result), and it writes below the next pass's first entry: the list is compacted in place
        for (int base = 0; __any(base < nsl); base += G) {
          const int idx = base + l;
          bool hit = idx < nsl; int pi = 0;
          if (hit) {  // the two bodies' bounding boxes (static geometry: axis-aligned in the world)
            pi = idx < MAXBPL ? S.bpl[idx] : tail[idx - MAXBPL];
            const int ba = sBP[2 * pi], bb = sBP[2 * pi + 1];
            const float* sa = S.bs[ba]; const float* sb = S.bs[bb];
            const float I9[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
            float Ra[9]; for (int k = 0; k < 9; k++) Ra[k] = static_code(ba) ? I9[k] : S.xR[ba][k];  // (side A is the static one of a pair, if any)
            hit = obb_face_overlap(sa, Ra, sBB + 8 * ba + 4, sb, S.xR[bb], sBB + 8 * bb + 4);
          }
          unsigned m16 = (unsigned)((__ballot(hit) >> (16 * r)) & 0xFFFFull);
          int pos = nbl + __popc(m16 & ((1u << l) - 1u));
          if (hit && pos < MAXBPL) S.bpl[pos] = (unsigned char)pi;
          nbl += __popc(m16);
          WSYNC();
        }
      }
#ifdef JH_V5_COUNT
      { const int nbm = wave_rowmax(nbl); if (lane == 0) V5_CADD(CB_BOXMAX, nbm); if (l == 0 && live) V5_CMAX(CB_MBOX, nbl); }
#endif
      if (nbl > MAXBPL) { if (l == 0 && live && stats) atomicAdd(stats + JH_STAT_DROPS, nbl - MAXBPL); nbl = MAXBPL; }  // (counted with the dropped contacts)
#ifdef JH_V5_COUNT
      if (l == 0 && live) cnt_bp += nbl;
#endif
      const int nh_cube = nh;
      WSYNC();
      V5_TICK(14)
      // level 2, per surviving body pair: (a) every geom of either body against the OTHER body's bounding box (one pass: lanes 0..nA-1 take A's geoms,
      // the next nB lanes B's; nA + nB <= 16) -- usually nothing of one side comes near the other and the pair is done; (b) the near geoms of A against
      // the near geoms of B (bounding spheres, then the six face axes of their boxes)
      for (int i = 0; __any(i < nbl); i++) {
#ifdef JH_V5_COUNT
        if (lane == 0) cnt_l2++;
#endif
        int ba = 0, bb = 0, ga0 = 0, na = 0, gb0 = 0, nb = 0;
        if (i < nbl) { const int pi = S.bpl[i]; ba = sBP[2 * pi]; bb = sBP[2 * pi + 1]; ga0 = sBG[2 * ba]; na = sBG[2 * ba + 1]; gb0 = sBG[2 * bb]; nb = sBG[2 * bb + 1]; }
        bool near = false;
        if (l < na + nb) {
          const bool isA = l < na;
          const int g = isA ? ga0 + l : gb0 + (l - na), own = isA ? ba : bb, oth = isA ? bb : ba;
          const float* gf = sGeomF + g * GEOM_F;
          float cw[3];
          if (static_code(own)) { cw[0] = gf[GF_POS]; cw[1] = gf[GF_POS + 1]; cw[2] = gf[GF_POS + 2]; }
          else { mulMV(cw, S.xR[own], gf + GF_POS); cw[0] += S.pa[own][0]; cw[1] += S.pa[own][1]; cw[2] += S.pa[own][2]; }
          const float dw[3] = {cw[0] - S.bs[oth][0], cw[1] - S.bs[oth][1], cw[2] - S.bs[oth][2]};
          float dl[3];
          if (static_code(oth)) { dl[0] = dw[0]; dl[1] = dw[1]; dl[2] = dw[2]; } else mulMTV(dl, S.xR[oth], dw);
          const float* hb = sBB + 8 * oth + 4;
          const float ex = fmaxf(fabsf(dl[0]) - hb[0], 0.f), ey = fmaxf(fabsf(dl[1]) - hb[1], 0.f), ez = fmaxf(fabsf(dl[2]) - hb[2], 0.f);
          near = ex * ex + ey * ey + ez * ez <= gf[GF_RBOUND] * gf[GF_RBOUND];
        }
        const unsigned m16 = (unsigned)((__ballot(near) >> (16 * r)) & 0xFFFFull);
        const unsigned mB = (m16 >> na) & ((1u << nb) - 1u);
        const unsigned mA = mB != 0 ? (m16 & ((1u << na) - 1u)) : 0u;
        const int nB = __popc(mB), T = __popc(mA) * nB;  // combinations (near geom of A, near geom of B) of this body pair
#ifdef JH_V5_COUNT
        {
          const int tm = wave_rowmax((T + G - 1) / G);
          if (lane == 0) V5_CADD(CB_COMBOPASS, tm);
          if (l == 0 && live && T != 0) { V5_CADD(CB_BPAIRS, 1); V5_CADD(CB_T, T); V5_CMAX(CB_MT, T); V5_CADD(CB_ONEA, __popc(mA) == 1); V5_CADD(CB_ONEB, nB == 1); V5_CADD(CB_OWNTRIPS, __popc(mA)); }
        }
#endif
        // (b) runs one lane per (near geom of A, near geom of B) combination, 16 per pass: combination t = ia' * nB + ib' (ia', ib': ranks among the near geoms of A and of B)
        // goes to lane t mod 16 of pass t / 16: ascending t is ascending geom of A, then ascending geom of B -- the order in which a loop over A's near geoms appends its survivors.  t / nB without a division: t < 256, nB <= 16, and (t + 0.5) / nB lies at least
        // 1 / 32 from an integer, far above the error of the reciprocal
        const float rnB = __builtin_amdgcn_rcpf((float)nB);
        for (int t = l; __any(t - l < T); t += G) {
          bool hit = false;
          int ga = 0, gb = 0;
          if (t < T) {
            const int ra = (int)(((float)t + 0.5f) * rnB), rb = t - ra * nB;
            ga = ga0 + nth_bit16(mA, ra); gb = gb0 + nth_bit16(mB, rb);
            const float* fa = sGeomF + ga * GEOM_F; const float* fb = sGeomF + gb * GEOM_F;
            float ca[3], cb[3];
            if (static_code(ba)) { ca[0] = fa[GF_POS]; ca[1] = fa[GF_POS + 1]; ca[2] = fa[GF_POS + 2]; }
            else { mulMV(ca, S.xR[ba], fa + GF_POS); ca[0] += S.pa[ba][0]; ca[1] += S.pa[ba][1]; ca[2] += S.pa[ba][2]; }
            mulMV(cb, S.xR[bb], fb + GF_POS); cb[0] += S.pa[bb][0]; cb[1] += S.pa[bb][1]; cb[2] += S.pa[bb][2];
            const float d[3] = {ca[0] - cb[0], ca[1] - cb[1], ca[2] - cb[2]}, rs = fa[GF_RBOUND] + fb[GF_RBOUND];
            hit = dot3(d, d) <= rs * rs;
            if (hit) {  // the geoms' own boxes (a sphere counts as the cube around it)
              float RA[9], RB[9];
              if (static_code(ba)) { for (int k = 0; k < 9; k++) RA[k] = fa[GF_R + k]; } else mulMM(RA, S.xR[ba], fa + GF_R);
              mulMM(RB, S.xR[bb], fb + GF_R);
#if JH_V5_CYL
              const int tyA = sGeomI[ga * GEOM_I + 1], tyB = sGeomI[gb * GEOM_I + 1];  // (a cylinder counts as the box (r, r, L) around it)
              const float hA[3] = {fa[GF_SIZE], tyA == GBOX ? fa[GF_SIZE + 1] : fa[GF_SIZE], tyA == GBOX ? fa[GF_SIZE + 2] : (tyA == GCYL ? fa[GF_SIZE + 1] : fa[GF_SIZE])};
              const float hB[3] = {fb[GF_SIZE], tyB == GBOX ? fb[GF_SIZE + 1] : fb[GF_SIZE], tyB == GBOX ? fb[GF_SIZE + 2] : (tyB == GCYL ? fb[GF_SIZE + 1] : fb[GF_SIZE])};
#else
              const bool sphA = sGeomI[ga * GEOM_I + 1] != GBOX, sphB = sGeomI[gb * GEOM_I + 1] != GBOX;
              const float hA[3] = {fa[GF_SIZE], sphA ? fa[GF_SIZE] : fa[GF_SIZE + 1], sphA ? fa[GF_SIZE] : fa[GF_SIZE + 2]};
              const float hB[3] = {fb[GF_SIZE], sphB ? fb[GF_SIZE] : fb[GF_SIZE + 1], sphB ? fb[GF_SIZE] : fb[GF_SIZE + 2]};
#endif
              hit = obb_face_overlap(ca, RA, hA, cb, RB, hB);
            }
          }
          const unsigned h16 = (unsigned)((__ballot(hit) >> (16 * r)) & 0xFFFFull);
          const int pos = nh + __popc(h16 & ((1u << l) - 1u));
          if (hit && pos < MAXHIT) S.hits[pos] = (unsigned short)(HITPAIR + (ga << 7 | gb));
          nh += __popc(h16);
        }
      }
#ifdef JH_V5_COUNT
      if (l == 0 && live) cnt_hh += nh - nh_cube;
#endif
      hand_hits = nh > nh_cube;
      }
      if (nh > MAXHIT) { if (l == 0 && live && stats) atomicAdd(stats + JH_STAT_DROPS, nh - MAXHIT); nh = MAXHIT; }  // (candidate pairs lost: counted with the dropped contacts)
      WSYNC();
      V5_TICK(1)
      // narrow phase: survivor i goes to lane i; side A is the cube or the first geom of a hand pair, side B a hand geom
      // (copies of a rollout in latency mode write the same values to the same row; the padding rows of the last workgroup -- n >= N, they recompute rollout N - 1 out of
      // lock step with the live row -- get no overflow row: their contacts above the LDS pool are dropped, and only live rows count what they drop)
      PoolCtx pc{&S, live ? stats : nullptr, (NOVF > 0 && ovf_all && n < N) ? ovf_all + (size_t)nc * (NOVF * POOL_F) : nullptr};
      for (int base = 0; __any(base < nh); base += G) {
        int idx = base + l;
        if (idx < nh) {
          const int hid = S.hits[idx];
          int ga = -1, gb = hid;
          if (SELF && hid >= HITPAIR) { ga = (hid - HITPAIR) >> 7; gb = (hid - HITPAIR) & 0x7F; }
          // side B
          const float* fb = sGeomF + gb * GEOM_F; const int bodyb = sGeomI[gb * GEOM_I], tb = sGeomI[gb * GEOM_I + 1];
          float pB[3], RB[9];
          if (bodyb < 0) { for (int k = 0; k < 3; k++) pB[k] = fb[GF_POS + k]; for (int k = 0; k < 9; k++) RB[k] = fb[GF_R + k]; }
          else { mulMV(pB, S.xR[bodyb], fb + GF_POS); for (int k = 0; k < 3; k++) pB[k] += S.pa[bodyb][k]; mulMM(RB, S.xR[bodyb], fb + GF_R); }
          // side A
          float pA[3], RA[9], hA[3], mua, trana; int ta, codea;
          if (!SELF || ga < 0) { for (int k = 0; k < 3; k++) { pA[k] = qc[k]; hA[k] = chs[k]; } for (int k = 0; k < 9; k++) RA[k] = Rc[k]; mua = 0.f; trana = ctran; ta = GBOX; codea = CUBE; }
          else {
            const float* fa = sGeomF + ga * GEOM_F; const int bodya = sGeomI[ga * GEOM_I];
            if (bodya < 0) { for (int k = 0; k < 3; k++) pA[k] = fa[GF_POS + k]; for (int k = 0; k < 9; k++) RA[k] = fa[GF_R + k]; }
            else { mulMV(pA, S.xR[bodya], fa + GF_POS); for (int k = 0; k < 3; k++) pA[k] += S.pa[bodya][k]; mulMM(RA, S.xR[bodya], fa + GF_R); }
            for (int k = 0; k < 3; k++) hA[k] = fa[GF_SIZE + k];
            mua = fa[GF_MUOWN]; trana = fa[GF_TRAN]; ta = sGeomI[ga * GEOM_I + 1]; codea = bodya < 0 ? 0 : bodya;
          }
          // contact parameters: friction = the larger of the two geoms' (the cube's is folded into GF_MU), R from the two bodies' inverse weights
          const float mu = (!SELF || ga < 0) ? fb[GF_MU] : fmaxf(mua, fb[GF_MUOWN]);
          LeapSink sk{pc, codea | ((bodyb < 0 ? 0 : bodyb) << 8), mu, trana + fb[GF_TRAN], false};
#if JH_V5_CYL
          // pairs with a cylinder.  The routines get the two geoms in MuJoCo's order (mj_collideGeoms: the geom of the lower type is geom 1; sphere 2 < cylinder 5 <
          // box 6), as the oracle's collision() has it; the pool stores the normal from side A to side B, so `flip` where that order swaps the sides.  The convex
          // routine gives at most one contact: a capturing sink, pushed here, keeps the pool's LDS atomics out of the non-inlined call.
          if (ta == GCYL || tb == GCYL) {
            const bool cylA = ta == GCYL;
            if ((cylA ? tb : ta) == GSPHERE) {  // cylinder-sphere (jh_coop.h: the primitive's normal runs from the cylinder to the sphere)
              if (cylA) collide_cylinder_sphere(sk, pA, RA, hA[0], hA[1], pB, fb[GF_SIZE]);
              else { sk.flip = true; collide_cylinder_sphere(sk, pB, RB, fb[GF_SIZE], fb[GF_SIZE + 1], pA, hA[0]); }
            } else {
              // geom 1 of the convex routine: the cylinder of a box-cylinder pair; of two cylinders, side A
              const bool swap = !cylA;
              CvxShape X{swap ? tb : ta, swap ? fb[GF_SIZE] : hA[0], swap ? fb[GF_SIZE + 1] : hA[1], swap ? fb[GF_SIZE + 2] : hA[2], {}, {}};
              CvxShape Y{swap ? ta : tb, swap ? hA[0] : fb[GF_SIZE], swap ? hA[1] : fb[GF_SIZE + 1], swap ? hA[2] : fb[GF_SIZE + 2], {}, {}};
              for (int k = 0; k < 3; k++) { X.p[k] = swap ? pB[k] : pA[k]; Y.p[k] = swap ? pA[k] : pB[k]; }
              for (int k = 0; k < 9; k++) { X.R[k] = swap ? RB[k] : RA[k]; Y.R[k] = swap ? RA[k] : RB[k]; }
              CvxOne one{{0.f, 0.f, 0.f}, {0.f, 0.f, 0.f}, 0.f, false};
              collide_convex_cylinder<CvxOne, CVX_STOP_NM>(one, X, Y);
              if (one.hit) { sk.flip = swap; sk.push(one.pos, one.n, one.dist); }
            }
          } else
#endif
          if ((!SELF || ta == GBOX) && tb == GBOX) collide_box_box(sk, pA, RA, hA, pB, RB, fb + GF_SIZE);
          else if (!SELF || ta == GBOX) collide_box_sphere(sk, pA, RA, hA, pB, fb[GF_SIZE]);
          else if (tb == GBOX) { sk.flip = true; collide_box_sphere(sk, pB, RB, fb + GF_SIZE, pA, hA[0]); }
          else {  // two spheres (fingertips)
            const float d[3] = {pB[0] - pA[0], pB[1] - pA[1], pB[2] - pA[2]}; const float dn = sqrtf(dot3(d, d)), dist = dn - hA[0] - fb[GF_SIZE];
            if (dist < 0.f && dn > 1e-9f) {
              const float n3[3] = {d[0] / dn, d[1] / dn, d[2] / dn}, m = hA[0] + 0.5f * dist;
              const float pos3[3] = {pA[0] + m * n3[0], pA[1] + m * n3[1], pA[2] + m * n3[2]};
              sk.push(pos3, n3, dist);
            }
          }
        }
      }
    }
    WSYNC();
    V5_TICK(2)
    // ================================================================ constraint rows: <= 2 contacts per lane + the own dof's friction-loss / limit rows
    // The constraint rows and the Newton solver exist once per slot count: a wave in which some rollout has more than 16 * NSLOT contacts this step (jammed cube:
    // several 4-point box-box manifolds at once) runs the copy with NSBIG slots per lane, all others the copy with NSLOT -- the third slot's 27 registers would
    // otherwise be spilled and reloaded inside every iteration of every rollout (measured: +17 % on the headline workload for 6e-4 of its rollout-steps).
    float a_own, ac_own; int iters_this = 0;
#ifdef JH_V5_CENSUS  // diagnostic builds (tools/diag/census_v5.py): histograms in stats[64..]: contacts per rollout-step / the maximum over the wave's rollouts, Newton iterations per
                     // rollout-step / per wave-step, line-search evaluations per Newton iteration of a rollout / of the wave, rollouts still active per Newton iteration of the wave
    const int wave_it0 = n_wave_iters;
    if (stats) {
      int mx = S.ncon; mx = max(mx, __shfl_xor(mx, 16)); mx = max(mx, __shfl_xor(mx, 32));
      if (l == 0 && live) atomicAdd(stats + 64 + min(S.ncon, 63), 1);
      if (lane == 0) atomicAdd(stats + 128 + min(mx, 63), 1);
      // (round 6) what a quad-per-contact assembly would need: cube contacts by the chain of their finger link (static geometry: any quad); passes = the longest quad's list
      int cn[5] = {0, 0, 0, 0, 0};
      const int ncc = S.ncon < NCP ? S.ncon : NCP;
      for (int i = 0; i < ncc; i++) { const int sd = __float_as_int(S.pool[i][8]), lb_ = sd >> 8; cn[(lb_ > 0 && lb_ < NMB) ? (lb_ - 1) >> 2 : 4]++; }
      const int cmx = max(max(cn[0], cn[1]), max(cn[2], cn[3])), tot_ = cn[0] + cn[1] + cn[2] + cn[3] + cn[4];
      int P = max(cmx, (tot_ + 3) >> 2), Pw = P; Pw = max(Pw, __shfl_xor(Pw, 16)); Pw = max(Pw, __shfl_xor(Pw, 32));
      int cw = cmx; cw = max(cw, __shfl_xor(cw, 16)); cw = max(cw, __shfl_xor(cw, 32));
      if (l == 0 && live) { atomicAdd(stats + 328 + min(P, 15), 1); atomicAdd(stats + 360 + min(cmx, 11), 1); }
      if (lane == 0) { atomicAdd(stats + 344 + min(Pw, 15), 1); atomicAdd(stats + 372 + min(cw, 11), 1); }
    }
#endif
    auto solve_step = [&](auto NS_, auto HC_) __attribute__((always_inline)) {
    constexpr bool HC = decltype(HC_)::value;  // hand contacts (a side that is not the cube) possible in this wave-step: false = the copy without their code (see the dispatch below)
    constexpr int NS = decltype(NS_)::value;
    const int ncap = (NOVF > 0 && (ovf_all == nullptr || n >= N) && 16 * NS > NCP) ? NCP : 16 * NS;  // (no overflow row: what the LDS pool holds)
    const int ncon = S.ncon < ncap ? S.ncon : ncap;
    Slot sl[NS];
    {
      float wv3[3]; mulMV(wv3, S.xR[0], vc + 3);  // world angular velocity of the cube
#pragma unroll
      for (int k = 0; k < NS; k++) {
        int idx = l + 16 * k;
        sl[k].la = -1; sl[k].lb = 0;
        for (int i = 0; i < 9; i++) sl[k].fr[i] = 0.f;
        sl[k].rc[0] = sl[k].rc[1] = sl[k].rc[2] = 0.f;
        sl[k].D0 = sl[k].D1 = sl[k].Dm = sl[k].mu = sl[k].fri = 0.f;  // (an empty slot is all zeros: the line search evaluates it like any other and gets zero, lane_rows_dir)
        for (int i = 0; i < 3; i++) sl[k].aref[i] = sl[k].jar[i] = sl[k].jp[i] = 0.f;
        if (idx < ncon) {
          const float* e = (NOVF == 0 || idx < NCP) ? S.pool[idx] : ovf_all + (size_t)nc * (NOVF * POOL_F) + (idx - NCP) * POOL_F;
          sl[k].rc[0] = e[0] - qc[0]; sl[k].rc[1] = e[1] - qc[1]; sl[k].rc[2] = e[2] - qc[2];
          sl[k].fr[0] = e[3]; sl[k].fr[1] = e[4]; sl[k].fr[2] = e[5];
          make_frame(sl[k].fr);
          float dist = e[6], mu = e[7], tran = e[9]; const int sides = __float_as_int(e[8]);
          sl[k].la = HC ? (sides & 0xFF) : CUBE; sl[k].lb = sides >> 8;
          float imp = impedance(csi, dist);
          float R0 = fmaxf(1e-15f, (1.f - imp) / imp * tran), R1 = R0 / fmaxf(1e-15f, impratio);
          sl[k].D0 = 1.f / R0; sl[k].D1 = 1.f / R1;
          sl[k].fri = mu; sl[k].mu = mu * sqrtf(R1 / R0);
          { float m2 = sl[k].mu * sl[k].mu; sl[k].Dm = sl[k].D0 / (m2 * (1.f + m2)); }
          float vel[3]; slot_Jx<HC>(sl[k], S, qc, vc, wv3, S.qv, vel);
          sl[k].aref[0] = -cB * vel[0] - cK * imp * dist; sl[k].aref[1] = -cB * vel[1]; sl[k].aref[2] = -cB * vel[2];
        }
      }
    }
    // The c3 cache: the joint columns axis_j x (pos - anchor_j) of the FIRST slot's side-B link (12 floats per lane, invariant over the Newton iterations of a step) are computed
    // once per step and kept in the part of the contact pool's storage the Newton matrices leave free (768 of 820 bytes): three ds_read_b128 per use instead of 24 loads +
    // 36 multiply-adds, twice per iteration.
    // (every lane has loaded its slots: the pool's storage is free from here on -- a wave's LDS instructions execute in order)
    if (sl[0].la >= 0 && sl[0].lb > 0) {
      const float pos0[3] = {sl[0].rc[0] + qc[0], sl[0].rc[1] + qc[1], sl[0].rc[2] + qc[2]};
      float c3[NLK][3]; link_c3(S, (sl[0].lb - 1) >> 2, pos0, c3);
      float4* o = reinterpret_cast<float4*>(S.c3s[l]);
      o[0] = make_float4(c3[0][0], c3[0][1], c3[0][2], c3[1][0]); o[1] = make_float4(c3[1][1], c3[1][2], c3[2][0], c3[2][1]); o[2] = make_float4(c3[2][2], c3[3][0], c3[3][1], c3[3][2]);
    }
#define V5_C3C(k) ((k) == 0 ? (const float*)S.c3s[l] : (const float*)nullptr)
    DofRows dr;
    dr.fl = lc[LC_FL]; dr.fD = lc[LC_FD]; dr.fR = dr.fD > 0.f ? 1.f / dr.fD : 0.f; dr.faref = -lc[LC_FB] * qd; dr.lims = 0.f; dr.laref = 0.f; dr.lD = 0.f; dr.jf = dr.jl = dr.pf = dr.pl = 0.f;
    if (lc[LC_LIMITED] != 0.f) {
      float dlo = q - lc[LC_LO], dhi = lc[LC_HI] - q, dist = fminf(dlo, dhi);
      if (dist < 0.f) {
        float sg = dlo < dhi ? 1.f : -1.f, imp = impedance(lc + LC_SI, dist), R = fmaxf(1e-15f, (1.f - imp) / imp * lc[LC_INVW]);
        dr.lims = sg; dr.lD = 1.f / R; dr.laref = -lc[LC_LB] * (sg * qd) - lc[LC_LK] * imp * dist;
      }
    }
    // Which finger chains are coupled by contacts between their links (hand self-collision): a 4 x 4 bit matrix per rollout, bit 4a + b for chains a < b.
    // Without a cycle in that graph (every coupled step of the headline workload: one pair, mostly middle-ring, or a chain touching both neighbours) the
    // arrow elimination runs in stages, leaf chains first: a chain is eliminated when at most one coupled neighbour is left (its parent `par`, whose
    // blocks take the Schur update and which factorises at a later stage `lvl`); then the cube.  A graph with a cycle takes the dense direction.
    bool anyslot = false; int cmask = 0; unsigned used = 0;
#pragma unroll
    for (int k = 0; k < NS; k++) {
      anyslot |= sl[k].la >= 0;
      used |= __any(sl[k].la >= 0) ? 1u << k : 0u;
      if (HC && sl[k].la > 0 && sl[k].la != CUBE && sl[k].lb > 0 && ((sl[k].la - 1) >> 2) != ((sl[k].lb - 1) >> 2)) cmask |= 1 << (4 * ((sl[k].la - 1) >> 2) + ((sl[k].lb - 1) >> 2));
    }
    int lvl = 0, par = -1, nlev = 0; bool dense_row = false;
    if constexpr (HC) {
      cmask = gor(cmask);
      if (__any(cmask != 0)) dense_row = !chain_elim_order(cmask, c, lvl, par, nlev);
#ifdef JH_V5_COUNT
      if (l == 0 && live) {
        int dmax = 0;
        for (int a = 0; a < NCH; a++) { int d = 0; for (int b = 0; b < NCH; b++) if (b != a) d += (cmask >> (a < b ? 4 * a + b : 4 * b + a)) & 1; dmax = d > dmax ? d : dmax; }
        cnt_cls[cmask == 0 ? 0 : (dense_row ? 3 : (dmax <= 1 ? 1 : 2))]++;
      }
#endif
    }
    S.pk_q[l] = q; S.pk_fs[l] = fs_own;
    if (l == 0) { S.pk_cq[0] = qc[3]; S.pk_cq[1] = qc[4]; S.pk_cq[2] = qc[5]; S.pk_cq[3] = qc[6]; S.pk_acc = acc; }
    // ================================================================ Newton solver (rows distributed over the 16 lanes)
    // The cube's three rotational dofs are solved for in WORLD coordinates (w = R w_body): with the cube's isotropic inertia (a cube: leap_cube, leap_cube_down,
    // caltech_leap_cube; checked at model load) the quadratic term is the same in both frames, and the rotation columns of a contact become e_q x r -- two non-zeros each --
    // instead of (R e_q) x r: no read of the cube's rotation matrix, no 3 x 3 product anywhere in a Newton iteration (gradient torque, Hessian columns, J p of the line
    // search).  The warm start and the integrated acceleration stay in the body frame (MuJoCo's free-joint convention): two 3 x 3 products per STEP.
    const float Mdiag_own = sel4(Mrow, s), iMd = 1.f / Mdiag_own;
    const float fsc_own = mck * a0c_own;
    const float snorm = gsum(fs_own * fs_own * iMd + fsc_own * fsc_own * lc[LC_IMCK]);
    const bool has_rows = gor((int)(anyslot || dr.fl > 0.f || dr.lims != 0.f)) != 0;
    iters_this = 0;
    if (!has_rows) { a_own = a0_own; ac_own = a0c_own; }
    else {
      // ---- warm start: the better of last step's acceleration (S.ws) and the unconstrained one
      {
        const float qws = S.ws[6 + l];
        float xl[3] = {S.ws[0], S.ws[1], S.ws[2]}, xr[3] = {S.ws[3], S.ws[4], S.ws[5]}, wa[3]; mulMV(wa, S.xR[0], xr);  // (S.ws keeps the body-frame acceleration of the last step)
        const float wsc_own = l < 3 ? S.ws[l] : (l == 3 ? wa[0] : (l == 4 ? wa[1] : (l == 5 ? wa[2] : 0.f)));
        float cs = 0.f, jx[3], jar_ws[NS][3];
#pragma unroll
        for (int k = 0; k < NS; k++) if (sl[k].la >= 0) {
          slot_Jx<HC>(sl[k], S, qc, xl, wa, S.ws, jx, V5_C3C(k));
          for (int rw = 0; rw < 3; rw++) { sl[k].jar[rw] = jx[rw] - sl[k].aref[rw]; jar_ws[k][rw] = sl[k].jar[rw]; }
          cs += cone_cost(sl[k]);
        }
        const float jf_ws = qws - dr.faref, jl_ws = dr.lims * qws - dr.laref;
        dr.jf = jf_ws; dr.jl = jl_ws;
        cs += dof_rows_cost(dr);
        float dws = qws - a0_own, md = 0.f;
#pragma unroll
        for (int j = 0; j < NLK; j++) md += Mrow[j] * (quad_get(qws, j) - quad_get(a0_own, j));
        cs += 0.5f * dws * md;
        { float dcw = wsc_own - a0c_own; cs += 0.5f * dcw * dcw * mck; }
        const float cost_ws = gsum(cs);
        S.p[6 + l] = a0_own; if (l < 6) S.p[l] = a0c_own;
        WSYNC();
        float xl0[3] = {S.p[0], S.p[1], S.p[2]}, xr0[3] = {S.p[3], S.p[4], S.p[5]};
        wa[0] = xr0[0]; wa[1] = xr0[1]; wa[2] = xr0[2];
        cs = 0.f;
#pragma unroll
        for (int k = 0; k < NS; k++) if (sl[k].la >= 0) {
          slot_Jx<HC>(sl[k], S, qc, xl0, wa, S.p, jx, V5_C3C(k));
          for (int rw = 0; rw < 3; rw++) sl[k].jar[rw] = jx[rw] - sl[k].aref[rw];
          cs += cone_cost(sl[k]);
        }
        dr.jf = a0_own - dr.faref; dr.jl = dr.lims * a0_own - dr.laref;
        cs += dof_rows_cost(dr);
        const float cost_0 = gsum(cs);
        if (cost_ws < cost_0) {
          a_own = qws; ac_own = wsc_own;
#pragma unroll
          for (int k = 0; k < NS; k++) if (sl[k].la >= 0) for (int rw = 0; rw < 3; rw++) sl[k].jar[rw] = jar_ws[k][rw];
          dr.jf = jf_ws; dr.jl = jl_ws;
        } else { a_own = a0_own; ac_own = a0c_own; }
        WSYNC();
      }
      bool act = true;
      V5_TICK(3)
      // The Newton loop exists twice: waves in which some rollout needs the dense direction this step run the copy that contains it, all others a copy
      // without that code (the register needs of the rare path would otherwise make the allocator spill inside every iteration of every rollout)
      auto forget_slots = [&]() __attribute__((always_inline)) {  // (the sides and the lever arm of every slot; not the frame: see the top of the file)
#pragma unroll
        for (int k = 0; k < NS; k++) { OPAQUE(sl[k].la); OPAQUE(sl[k].lb); OPAQUE(sl[k].rc[0]); OPAQUE(sl[k].rc[1]); OPAQUE(sl[k].rc[2]); }
      };
      auto newton_loop = [&](auto dense_tag) __attribute__((always_inline)) {
      constexpr bool DENSE = decltype(dense_tag)::value;
      for (int it = 0; it < cap && __any(act); it++) {
        // ---- (1) gradient.  Owner lanes: M (a - a0) rows + dof-row forces; contacts: -J'f as LDS float atomics (finger and cube parts)
        forget_slots();
        const float da_own = a_own - a0_own, dcl = ac_own - a0c_own;
        float g_own = 0.f, hd = 0.f;
#pragma unroll
        for (int j = 0; j < NLK; j++) g_own += Mrow[j] * quad_get(da_own, j);
        {  // the own dof's friction-loss and limit rows (selects: see lane_rows_dir)
          const float D = dr.fD, x = dr.jf, fl = dr.fl, lim = dr.fR * fl;
          const bool has = fl > 0.f, lo_ = x <= -lim, hi_ = x >= lim, mid = has & !lo_ & !hi_;
          float ga = g_own - fl, gb = g_own + fl, gm = fmaf(D, x, g_own); asm volatile("" : "+v"(ga), "+v"(gb), "+v"(gm));  // (all three computed: selects, not branches)
          g_own = has ? (lo_ ? ga : (hi_ ? gb : gm)) : g_own;
          hd = mid ? hd + D : hd;
          const bool lon = (dr.lims != 0.f) & (dr.jl < 0.f);
          g_own = lon ? fmaf(dr.lims * dr.lD, dr.jl, g_own) : g_own;
          hd = lon ? hd + dr.lD : hd;
        }
        S.g[6 + l] = g_own;  // (this and the block initialisation below are stored whatever the rollout's state -- nothing of a converged rollout is read again this step, a dense
                             // row's matrix is zeroed after them -- so that the top of an iteration has no exec-masked region in front of the contact pass)
        // One pass over the contacts builds the gradient AND the Hessian of this iterate: the joint columns axis x (pos - anchor), the world force and the cone weights are
        // computed once instead of once per pass.  The pass that finds a rollout converged has then assembled a Hessian nobody reads (one iteration in ten).
        const bool aact0 = act && !(DENSE && dense_row);
        {
          float* hb = &S.Hbb[c][tri(s, 0)];  // row s of the chain's block: entries j < s, then the diagonal -- written once per column index j, the columns beyond the diagonal land on it again
#pragma unroll
          for (int j = 0; j < NLK; j++) hb[j < s ? j : s] = j < s ? Mrow[j] : Mdiag_own + hd;
          for (int k = 0; k < 6; k++) S.Hcb[c][s * 6 + k] = 0.f;
          if (HC) for (int k = 0; k < 6; k++) S.Hx[0][l * 6 + k] = 0.f;
        }
        float hcp[21];  // the cube block J'WJ of this lane's contacts: every cube contact of the rollout lands on the same 21 entries -> row sums instead of 21 conflicting atomics per contact
#pragma unroll
        for (int e = 0; e < 21; e++) hcp[e] = 0.f;
        bool hcany = false;
        WSYNC();
        float gcp[6] = {0, 0, 0, 0, 0, 0};  // cube part of -J'f: every contact of the rollout lands on the same six entries -> row sums, not atomics
        {
#pragma unroll
          for (int k = 0; k < NS; k++) {
            if (k > 0 && !((used >> k) & 1u)) continue;  // (wave-uniform)
            const Slot& t = sl[k];
            float f[3], Wk[6];
            const float D[3] = {t.D0, t.D1, t.D1};
            // separated contact (the cone's top zone: no force, no weights): skipped on the zone test itself, before any of the other zones' arithmetic.  (The other two zones have
            // a positive W[0]: `weights all zero` and `top zone` are the same set of contacts.)  Outside the dense-capable copy `aact0` is `act`, true in here: `on` is a
            // compile-time constant there
            // One exec-masked region per slot: an empty slot is all zeros and reads `top`, a converged rollout is masked by the same test.
            ConeZ cz;
            if (cone_top(t.jar, t.mu, t.fri, cz) | !act) continue;
            cone_below(t.jar, D, t.Dm, t.mu, t.fri, cz, f, Wk);
            bool on = true;
            if constexpr (DENSE) on = aact0;
            const float Fw[3] = {t.fr[0] * f[0] + t.fr[3] * f[1] + t.fr[6] * f[2], t.fr[1] * f[0] + t.fr[4] * f[1] + t.fr[7] * f[2], t.fr[2] * f[0] + t.fr[5] * f[1] + t.fr[8] * f[2]};
            const float pos[3] = {t.rc[0] + qc[0], t.rc[1] + qc[1], t.rc[2] + qc[2]};
            const bool cube = !HC || t.la == CUBE;
            // J'WJ in the world frame: every dof column of the contact is a world 3-vector col_x (J[w][x] = fr_w . col_x), so the entry (x, y) is col_x' A col_y with
            // A = Fr' W Fr, a symmetric 3 x 3 formed once per contact.  The cube's translation columns are -e_q: their block is A itself and their coupling to a column c is
            // -(A c)_q, both free; a third fewer multiply-adds than frame-space columns times W (the fr3 kernel's formulation).
            float A[6];
            if (on) {
              float T0[3], T1[3], T2[3];
#pragma unroll
              for (int q = 0; q < 3; q++) {
                T0[q] = Wk[0] * t.fr[q] + Wk[1] * t.fr[3 + q] + Wk[3] * t.fr[6 + q];
                T1[q] = Wk[1] * t.fr[q] + Wk[2] * t.fr[3 + q] + Wk[4] * t.fr[6 + q];
                T2[q] = Wk[3] * t.fr[q] + Wk[4] * t.fr[3 + q] + Wk[5] * t.fr[6 + q];
              }
#pragma unroll
              for (int i = 0; i < 3; i++)
#pragma unroll
                for (int j = 0; j <= i; j++) A[tri(i, j)] = t.fr[i] * T0[j] + t.fr[3 + i] * T1[j] + t.fr[6 + i] * T2[j];
            }
            auto Amul = [&](const float* v, float* y) __attribute__((always_inline)) {
              y[0] = A[0] * v[0] + A[1] * v[1] + A[3] * v[2]; y[1] = A[1] * v[0] + A[2] * v[1] + A[4] * v[2]; y[2] = A[3] * v[0] + A[4] * v[1] + A[5] * v[2];
            };
            if (cube) {
              float tb[3]; cross3(tb, t.rc, Fw);  // torque about the cube's origin, world
              gcp[0] += Fw[0]; gcp[1] += Fw[1]; gcp[2] += Fw[2]; gcp[3] += tb[0]; gcp[4] += tb[1]; gcp[5] += tb[2];
              if (on) {
#pragma unroll
                for (int e = 0; e < 6; e++) hcp[e] += A[e];
                // rotation columns e_q x r = (0, -rz, ry), (rz, 0, -rx), (-ry, rx, 0): z_q = A (e_q x r) is a combination of two columns of A, and a dot product with
                // e_p x r has two terms
                const float rx = t.rc[0], ry = t.rc[1], rz = t.rc[2];
                const float Ac[3][3] = {{A[0], A[1], A[3]}, {A[1], A[2], A[4]}, {A[3], A[4], A[5]}};  // column k of A (symmetric)
                float zq[3][3];
#pragma unroll
                for (int i = 0; i < 3; i++) { zq[0][i] = ry * Ac[2][i] - rz * Ac[1][i]; zq[1][i] = rz * Ac[0][i] - rx * Ac[2][i]; zq[2][i] = rx * Ac[1][i] - ry * Ac[0][i]; }
#pragma unroll
                for (int q = 0; q < 3; q++) {
#pragma unroll
                  for (int r2 = 0; r2 < 3; r2++) hcp[tri(3 + q, r2)] += zq[q][r2];
                }
                hcp[tri(3, 3)] += ry * zq[0][2] - rz * zq[0][1];
                hcp[tri(4, 3)] += ry * zq[1][2] - rz * zq[1][1]; hcp[tri(4, 4)] += rz * zq[1][0] - rx * zq[1][2];
                hcp[tri(5, 3)] += ry * zq[2][2] - rz * zq[2][1]; hcp[tri(5, 4)] += rz * zq[2][0] - rx * zq[2][2]; hcp[tri(5, 5)] += rx * zq[2][1] - ry * zq[2][0];
                hcany = true;
              }
            }
            if (t.lb > 0) {
              const int ch = (t.lb - 1) >> 2, dep = (t.lb - 1) & 3;
              const bool linkA = HC && !cube && t.la > 0;
              const int cha = linkA ? (t.la - 1) >> 2 : 0, depa = linkA ? (t.la - 1) & 3 : -1;
              const bool same = linkA && cha == ch;
              float cb[NLK][3]; if (V5_C3C(k)) load_c3(V5_C3C(k), cb); else link_c3(S, ch, pos, cb);
              if constexpr (!HC) {
                // cube contact on a finger link (the copy without the hand's own contacts): joint u4 of the chain carries the contact iff u4 <= dep -- its gradient entry, its row
                // of the chain block and its coupling to the cube under ONE test per joint (the general form below: one for the force, one for the rows, and the columns
                // beyond the link's depth zeroed first -- here they are never read)
#pragma unroll
                for (int u4 = 0; u4 < NLK; u4++) if (u4 <= dep) {
                  atomicAdd(&S.g[6 + 4 * ch + u4], -dot3(cb[u4], Fw));
                  float y[3]; Amul(cb[u4], y);
#pragma unroll
                  for (int v4 = 0; v4 <= u4; v4++) atomicAdd(&S.Hbb[ch][tri(u4, v4)], dot3(cb[v4], y));
#pragma unroll
                  for (int q = 0; q < 3; q++) atomicAdd(&S.Hcb[ch][u4 * 6 + q], -y[q]);
                  atomicAdd(&S.Hcb[ch][u4 * 6 + 3], t.rc[2] * y[1] - t.rc[1] * y[2]);  // -(e_q x r) . y
                  atomicAdd(&S.Hcb[ch][u4 * 6 + 4], t.rc[0] * y[2] - t.rc[2] * y[0]);
                  atomicAdd(&S.Hcb[ch][u4 * 6 + 5], t.rc[1] * y[0] - t.rc[0] * y[1]);
                }
              } else {
              // (the hand-capable copy as the other one: a joint's gradient entry, its row of the chain block and its coupling to the cube under ONE test per joint; the
              // coupling of a contact that is not the cube's is added as zeros instead of sitting in a nested exec-masked region per joint; the opposite force of a contact with both
              // sides in one chain -- rare -- behind one wave-uniform test.  The same values reach the same addresses in the same order.)
              float fjs[NLK];
#pragma unroll
              for (int u4 = 0; u4 < NLK; u4++) {
                fjs[u4] = dot3(cb[u4], Fw);
                const float sg = (u4 <= dep ? 1.f : 0.f) - ((same && u4 <= depa) ? 1.f : 0.f);
                cb[u4][0] *= sg; cb[u4][1] *= sg; cb[u4][2] *= sg;
                if (u4 <= dep) {
                  atomicAdd(&S.g[6 + 4 * ch + u4], -fjs[u4]);  // side B: -J'f
                  if (on) {
                    float y[3]; Amul(cb[u4], y);
#pragma unroll
                    for (int v4 = 0; v4 <= u4; v4++) atomicAdd(&S.Hbb[ch][tri(u4, v4)], dot3(cb[v4], y));
                    const float hv[6] = {-y[0], -y[1], -y[2], t.rc[2] * y[1] - t.rc[1] * y[2], t.rc[0] * y[2] - t.rc[2] * y[0], t.rc[1] * y[0] - t.rc[0] * y[1]};  // -(e_q x r) . y
                    if (cube) {
#pragma unroll
                      for (int q = 0; q < 6; q++) atomicAdd(&S.Hcb[ch][u4 * 6 + q], hv[q]);
                    }
                  }
                }
              }
              if (__any(same)) {
#pragma unroll
                for (int j = 0; j < NLK; j++) if (same && j <= depa) atomicAdd(&S.g[6 + 4 * ch + j], fjs[j]);  // side A of the same chain: the opposite force
              }
              if (linkA && !same) {  // side A sits in another chain: its own block, and the pair's coupling block -Jb'W Ja in Hx (B's chain is always the higher one)
                float ca[NLK][3]; link_c3(S, cha, pos, ca);
#pragma unroll
                for (int j = 0; j < NLK; j++) {
                  if (j <= depa) atomicAdd(&S.g[6 + 4 * cha + j], dot3(ca[j], Fw));
                  const float sg = j <= depa ? 1.f : 0.f;
                  ca[j][0] *= sg; ca[j][1] *= sg; ca[j][2] *= sg;
                }
                if (on) {
#pragma unroll
                  for (int u4 = 0; u4 < NLK; u4++) if (u4 <= depa) {
                    float y[3]; Amul(ca[u4], y);
#pragma unroll
                    for (int v4 = 0; v4 <= u4; v4++) atomicAdd(&S.Hbb[cha][tri(u4, v4)], dot3(ca[v4], y));
#pragma unroll
                    for (int v4 = 0; v4 < NLK; v4++) if (v4 <= dep) atomicAdd(&S.Hx[pidx(cha, ch)][v4 * 4 + u4], -dot3(cb[v4], y));
                  }
                }
              }
              }
            }
          }
        }
        float gcl = 0.f;
        float h0 = 0.f, h1;
        {  // two reduce-scatters: entries 16..20 of the cube block (to lanes 0..4) with the six gradient sums (to lanes 8..13, moved to 0..5 by a rotation), and entries 0..15
          const float v2[16] = {hcp[16], hcp[17], hcp[18], hcp[19], hcp[20], 0.f, 0.f, 0.f, gcp[0], gcp[1], gcp[2], gcp[3], gcp[4], gcp[5], 0.f, 0.f};
          h1 = row_scatter16(v2, l);
          const float gq = dppf<0x128>(h1);
          gcl = l < 6 ? gq : 0.f;
          if (__any(hcany)) h0 = row_scatter16(hcp, l);
        }
        gcl = fmaf(mck, dcl, gcl);
        {
          // (stored whatever the rollout's state: nothing of a converged rollout is read again this step, and a dense row's matrix is zeroed after this.  The cube's own
          // mass diagonal is added where the block is read back: no LDS read -- a round trip behind the atomics above -- between the sums and the convergence test)
          // (addressed from the lane's gradient entry, the address the next statement reads: the hand-capable copy had `&S.Hcc[l]` spilled to scratch memory -- a reload
          // and its wait between the sums and the convergence test)
          constexpr int HCC_G = ((int)offsetof(RS, Hcc) - (int)offsetof(RS, g)) / 4 - 6;
          float* gl = &S.g[6 + l];
          gl[HCC_G] = h0;
          if (l < 5) gl[HCC_G + 16] = h1;
        }
        WSYNC();
        V5_TICK(4)
        // ---- (2) convergence on the scaled gradient; the wave leaves the loop before any Hessian work once all its rollouts are done
        g_own = S.g[6 + l];
        const float gn = gsum(g_own * g_own * iMd + gcl * gcl * lc[LC_IMCK]);
        act = act & !(gn <= tol * tol * fmaxf(snorm, 1e-12f));
        if (!__any(act)) break;
        iters_this += act ? 1 : 0;
        n_wave_iters++;
        // ---- (3) Hessian: M + dof rows on the chain diagonals, cube inertia on Hcc, J'WJ of the contacts as atomics into the arrow blocks.  A rollout with a
        // contact between two finger chains has no arrow structure: its Hessian is assembled densely further down (aact = false here)
        const bool aact = act && !(DENSE && dense_row);
        V5_TICK(5)
        // ---- (4) arrow factorisation: chain blocks first (each chain's 4 lanes redundantly); the coupling columns Y_q = L^-1 Hcb[:,q] are shared
        // by the chain's lanes (lane s: columns s and s+4); 6x6 Schur complement on the cube, solved by every lane
        float L[10], Linv[4], Ya[NLK], Yb[NLK], zb[NLK], xc6[6], pc4[NLK];
        const bool hasb = s < 2;  // lanes 0,1 of a chain carry a second column (q = 4, 5)
        auto factor_block = [&]() __attribute__((always_inline)) {
          for (int k = 0; k < 10; k++) L[k] = S.Hbb[c][k];
          chol4(L, Linv);
          for (int j = 0; j < NLK; j++) { Ya[j] = S.Hcb[c][j * 6 + s]; const float yb = (&S.Hcb[0][0])[c * 24 + j * 6 + 4 + (s & 1)]; Yb[j] = hasb ? yb : 0.f; }  // (unconditional load, then select)
          fwd4(L, Linv, Ya); fwd4(L, Linv, Yb);
          asm volatile("" : "+v"(Yb[0]), "+v"(Yb[1]), "+v"(Yb[2]), "+v"(Yb[3]));  // (the compiler forgets that they are zero where `hasb` is false: it split everything downstream into a copy per case, and a quad runs both)
          for (int j = 0; j < NLK; j++) zb[j] = -S.g[6 + 4 * c + j];
          fwd4(L, Linv, zb);
        };
        factor_block();
        if (l < 6) S.rhs6[l] = -gcl;
        float Xs[NLK] = {0.f, 0.f, 0.f, 0.f};  // column s of X = L^-1 H(a,P) of a chain a with a parent P
        if constexpr (HC) {
#pragma unroll 1
          for (int st = 1; st < NCH; st++) {
            if (!__any(aact && nlev >= st)) break;
            // chains of stage st - 1 with a parent: their elimination updates the parent's blocks -- Hbb(P) -= X'X, Hcb(P) -= X'Y, g(P) += X'zb (so that the
            // parent's zb becomes L_P^-1 (-g_P - X'zb_a)) -- before the parent factorises at its own stage (atomics: two leaves may share a parent)
            const bool me = aact && lvl == st - 1 && par >= 0;
            if (me) {
              const float* hx = par > c ? S.Hx[pidx(c, par)] : S.Hx[pidx(par, c)];
              for (int j = 0; j < NLK; j++) Xs[j] = par > c ? hx[s * 4 + j] : hx[j * 4 + s];  // H(a,P)[ia = j][iP = s]
              fwd4(L, Linv, Xs);
            }
#pragma unroll
            for (int j = 0; j < NLK; j++) {
              const float v = Xs[0] * quad_get(Xs[0], j) + Xs[1] * quad_get(Xs[1], j) + Xs[2] * quad_get(Xs[2], j) + Xs[3] * quad_get(Xs[3], j);
              if (me && j <= s) atomicAdd(&S.Hbb[par][tri(s, j)], -v);
            }
#pragma unroll
            for (int q6 = 0; q6 < 6; q6++) {
              float v = 0.f;
#pragma unroll
              for (int j = 0; j < NLK; j++) v += Xs[j] * (q6 < 4 ? quad_get(Ya[j], q6) : quad_get(Yb[j], q6 - 4));
              if (me) atomicAdd(&S.Hcb[par][s * 6 + q6], -v);
            }
            if (me) atomicAdd(&S.g[6 + 4 * par + s], Xs[0] * zb[0] + Xs[1] * zb[1] + Xs[2] * zb[2] + Xs[3] * zb[3]);
            WSYNC();
            if (lvl == st) factor_block();  // the updated blocks
          }
        }
        WSYNC();
        V5_TICK(6)
        {
          // Schur complement: Hcc[q][r] -= sum over chains of Y_q . Y_r, rhs6[q] -= sum of Y_q . zb; lane s of a chain owns q in {s, s+4} and fetches Y_r from
          // its chain-mates; the four chains' terms are added with two row rotations and the first chain's lane applies the total
          float dar[6], dbr[6];  // the four chains' terms of row s (dar) and row 4 + s (dbr), column r6, summed over the chains: the same numbers in every chain's lane s
#pragma unroll
          for (int r6 = 0; r6 < 6; r6++) {
            float Yr[NLK];
#pragma unroll
            for (int j = 0; j < NLK; j++) Yr[j] = r6 < 4 ? quad_get(Ya[j], r6) : quad_get(Yb[j], r6 - 4);
            float da = Ya[0] * Yr[0] + Ya[1] * Yr[1] + Ya[2] * Yr[2] + Ya[3] * Yr[3], db = Yb[0] * Yr[0] + Yb[1] * Yr[1] + Yb[2] * Yr[2] + Yb[3] * Yr[3];
            dar[r6] = qsum4_same(da); dbr[r6] = qsum4_same(db);
            continue;
            da = qsum4(da); db = qsum4(db);
            const bool app = aact && c == 0;
            if (app) {
              // (LDS atomics, not `S.Hcc[..] -= da`: the compiler cannot prove the addresses distinct and turns every read-modify-write into its own LDS round trip --
              // ds_read, wait, ds_write -- fourteen of them in a row per iteration; x + (-da) is the same number, and ds_add_f32 is not waited for: 78.4 against 79.4 ms)
              if (r6 <= s) atomicAdd(&S.Hcc[tri(s, r6)], -da);
              if (hasb && r6 <= 4 + s) atomicAdd(&S.Hcc[tri(4 + s, r6)], -db);
            }
          }
          float ra = Ya[0] * zb[0] + Ya[1] * zb[1] + Ya[2] * zb[2] + Ya[3] * zb[3], rb = Yb[0] * zb[0] + Yb[1] * zb[1] + Yb[2] * zb[2] + Yb[3] * zb[3];
          ra = qsum4_same(ra); rb = qsum4_same(rb);
          // the complement stays in registers: every lane needs all of it for the redundant 6 x 6 solve anyway -- 27 quad broadcasts instead of 27 atomics, a fence and
          // the wait for them
          float Lc[21];
#pragma unroll
          for (int q6 = 0; q6 < 6; q6++) {
#pragma unroll
            for (int r6 = 0; r6 <= q6; r6++) Lc[tri(q6, r6)] = (r6 == q6 ? S.Hcc[tri(q6, r6)] + S.cmd[q6 < 3 ? 0 : q6 - 2] : S.Hcc[tri(q6, r6)]) - (q6 < 4 ? quad_get(dar[r6], q6) : quad_get(dbr[r6], q6 - 4));
            xc6[q6] = S.rhs6[q6] - (q6 < 4 ? quad_get(ra, q6) : quad_get(rb, q6 - 4));
          }
          float ci[6];
#pragma unroll
          for (int i = 0; i < 6; i++)
#pragma unroll
            for (int j = 0; j <= i; j++) {
              float sv = Lc[tri(i, j)];
#pragma unroll
              for (int k = 0; k < j; k++) sv -= Lc[tri(i, k)] * Lc[tri(j, k)];
              if (i == j) { float rr = __frsqrt_rn(fmaxf(sv, 1e-30f)); ci[i] = rr; Lc[tri(i, i)] = sv * rr; }
              else Lc[tri(i, j)] = sv * ci[j];
            }
#pragma unroll
          for (int i = 0; i < 6; i++) { float sv = xc6[i];
#pragma unroll
            for (int k = 0; k < i; k++) sv -= Lc[tri(i, k)] * xc6[k];
            xc6[i] = sv * ci[i]; }
#pragma unroll
          for (int i = 5; i >= 0; i--) { float sv = xc6[i];
#pragma unroll
            for (int k = i + 1; k < 6; k++) sv -= Lc[tri(k, i)] * xc6[k];
            xc6[i] = sv * ci[i]; }
          // back-substitution through the coupling: pc = L^-T (zb - sum_q Y_q x_q); each lane contributes its columns, summed over the chain
          asm volatile("" : "+v"(xc6[0]), "+v"(xc6[1]), "+v"(xc6[2]), "+v"(xc6[3]), "+v"(xc6[4]), "+v"(xc6[5]));  // (the solution is complete in every lane before anything is picked from it: the picks stay selects)
          float xa = sel4o(xc6, s), xb = s == 0 ? xc6[4] : xc6[5]; asm volatile("" : "+v"(xb));
#pragma unroll
          for (int j = 0; j < NLK; j++) pc4[j] = zb[j] - csum(fmaf(Ya[j], xa, Yb[j] * xb));  // (Yb is zero in the lanes without a second column)
          if constexpr (HC) {
            if (__any(aact && nlev > 0)) {
              // p_a = L_a^-T (zb_a - Y_a x_c - X p_P): parents finish first (last stage first) and publish their part of the direction
#pragma unroll 1
              for (int st = NCH - 1; st >= 0; st--) {
                if (!__any(aact && nlev >= st)) continue;
                const bool me = aact && lvl == st;
                const float pbs = (me && par >= 0) ? S.p[6 + 4 * par + s] : 0.f;
#pragma unroll
                for (int j = 0; j < NLK; j++) pc4[j] -= csum(Xs[j] * pbs);
                if (st > 0) {
                  float pb4[NLK];
                  for (int j = 0; j < NLK; j++) pb4[j] = pc4[j];
                  bwd4(L, Linv, pb4);
                  if (me) S.p[6 + l] = sel4(pb4, s);
                  WSYNC();
                }
              }
            }
          }
          bwd4(L, Linv, pc4);
        }
        asm volatile("" : "+v"(pc4[0]), "+v"(pc4[1]), "+v"(pc4[2]), "+v"(pc4[3]));
        float p_own = sel4o(pc4, s);
        float xcl;  // own entry of the cube's part of the direction (lanes 0..5), zero elsewhere: selects with opaque results (see sel4o)
        { float x03 = sel4o(xc6, l & 3), x45 = (l & 1) ? xc6[5] : xc6[4]; asm volatile("" : "+v"(x45)); xcl = l < 4 ? x03 : (l < 6 ? x45 : 0.f); asm volatile("" : "+v"(xcl)); }
        S.p[6 + l] = p_own; if (l < 6) S.p[l] = xcl;
        WSYNC();
        // ---- (4b) dense path: rollouts with a contact between two finger chains (hand self-collision; rare).  H = M + J'WJ as a packed 22 x 22 matrix in
        // LDS, Cholesky by rows in registers and the two triangular solves with the rollout's 16 lanes (rows l and l + 16)
        if constexpr (HC && DENSE) {
#ifdef JH_V5_COUNT
        if (lane == 0) { cnt_it++; cnt_dense += __any(act && dense_row) ? 1 : 0; }
#endif
        if (__any(act && dense_row)) {
          const bool dact = act && dense_row;
          if (dact) for (int e = l; e < NDH; e += G) S.Hd[e] = 0.f;
          WSYNC();
          if (dact) {
#pragma unroll
            for (int j = 0; j < NLK; j++) if (j <= s) S.Hd[tri(6 + l, 6 + 4 * c + j)] = Mrow[j] + (j == s ? hd : 0.f);
            if (l < 6) { S.Hd[tri(l, l)] = mck; S.g[l] = gcl; }
          }
          WSYNC();
#pragma unroll
          for (int k = 0; k < NS; k++) {
            const Slot& t = sl[k];
            if (!(dact && t.la >= 0)) continue;
            float f[3], Wk[6];
            const float D[3] = {t.D0, t.D1, t.D1};
            cone_eval(t.jar, D, t.Dm, t.mu, t.fri, f, Wk);
            if (Wk[0] == 0.f && Wk[2] == 0.f && Wk[5] == 0.f) continue;
            const float pos[3] = {t.rc[0] + qc[0], t.rc[1] + qc[1], t.rc[2] + qc[2]};
            // three column blocks: X0 = cube (6 columns at dof 0) or side-A link (4 columns at its chain), X1 = side-B link (4 columns)
            float X0[6][3], X1[NLK][3];
            for (int j = 0; j < 6; j++) X0[j][0] = X0[j][1] = X0[j][2] = 0.f;
            for (int j = 0; j < NLK; j++) X1[j][0] = X1[j][1] = X1[j][2] = 0.f;
            int o0 = 0, n0 = 0, o1 = 0, n1 = 0;
            if (t.la == CUBE) {
              n0 = 6;
              for (int q3 = 0; q3 < 3; q3++) {
                X0[q3][0] = -t.fr[q3]; X0[q3][1] = -t.fr[3 + q3]; X0[q3][2] = -t.fr[6 + q3];
                const float ea[3] = {q3 == 0 ? 1.f : 0.f, q3 == 1 ? 1.f : 0.f, q3 == 2 ? 1.f : 0.f}; float c3[3]; cross3(c3, ea, t.rc);
                X0[3 + q3][0] = -dot3(t.fr, c3); X0[3 + q3][1] = -dot3(t.fr + 3, c3); X0[3 + q3][2] = -dot3(t.fr + 6, c3);
              }
            } else if (t.la > 0) { o0 = 6 + 4 * ((t.la - 1) >> 2); n0 = 1 + ((t.la - 1) & 3); link_cols(S, t.la, pos, t.fr, -1.f, X0); }
            if (t.lb > 0) {
              o1 = 6 + 4 * ((t.lb - 1) >> 2); n1 = 1 + ((t.lb - 1) & 3);
              if (t.la != CUBE && t.la > 0 && o1 == o0) { link_cols(S, t.lb, pos, t.fr, 1.f, X0); n0 = n0 > n1 ? n0 : n1; n1 = 0; }  // same chain: one block
              else link_cols(S, t.lb, pos, t.fr, 1.f, X1);
            }
            if (n1 > 0 && n0 > 0 && o1 < o0) {  // keep the blocks in dof order (X0 before X1) so that every entry lands in the lower triangle
              for (int j = 0; j < NLK; j++) for (int q = 0; q < 3; q++) { const float tmp = X0[j][q]; X0[j][q] = X1[j][q]; X1[j][q] = tmp; }
              int ti = o0; o0 = o1; o1 = ti; ti = n0; n0 = n1; n1 = ti;
            }
#pragma unroll
            for (int u = 0; u < 6; u++) if (u < n0) {
              const float* j3 = X0[u];
              const float G0 = Wk[0] * j3[0] + Wk[1] * j3[1] + Wk[3] * j3[2], G1 = Wk[1] * j3[0] + Wk[2] * j3[1] + Wk[4] * j3[2], G2 = Wk[3] * j3[0] + Wk[4] * j3[1] + Wk[5] * j3[2];
#pragma unroll
              for (int v = 0; v <= u; v++) atomicAdd(&S.Hd[tri(o0 + u, o0 + v)], X0[v][0] * G0 + X0[v][1] * G1 + X0[v][2] * G2);
#pragma unroll
              for (int v = 0; v < NLK; v++) if (v < n1) atomicAdd(&S.Hd[tri(o1 + v, o0 + u)], X1[v][0] * G0 + X1[v][1] * G1 + X1[v][2] * G2);
            }
#pragma unroll
            for (int u = 0; u < NLK; u++) if (u < n1) {
              const float* j3 = X1[u];
              const float G0 = Wk[0] * j3[0] + Wk[1] * j3[1] + Wk[3] * j3[2], G1 = Wk[1] * j3[0] + Wk[2] * j3[1] + Wk[4] * j3[2], G2 = Wk[3] * j3[0] + Wk[4] * j3[1] + Wk[5] * j3[2];
#pragma unroll
              for (int v = 0; v <= u; v++) atomicAdd(&S.Hd[tri(o1 + u, o1 + v)], X1[v][0] * G0 + X1[v][1] * G1 + X1[v][2] * G2);
            }
          }
          WSYNC();
          // Cholesky by rows: lane l keeps rows l and 16 + l (l < 6) of the factor in registers.  Column k: every lane reads row k's finished entries
          // L[k][0..k-1] from LDS (published as they were finished), forms the pivot redundantly and finishes its own rows' entry of column k --
          // one LDS round trip per column, all reads of a column independent of each other
          const int r1 = 16 + l;
          const bool two = l < 6;
          float h0[16], h1[NV];
#pragma unroll
          for (int j = 0; j < 16; j++) h0[j] = (dact && j <= l) ? S.Hd[tri(l, j)] : 0.f;
#pragma unroll
          for (int j = 0; j < NV; j++) h1[j] = (dact && two && j <= r1) ? S.Hd[tri(r1, j)] : 0.f;
#pragma unroll
          for (int kk = 0; kk < NV; kk++) {
            float dp = 0.f, s0 = kk < 16 ? h0[kk < 16 ? kk : 0] : 0.f, s1 = h1[kk];
            const float hkk = dact ? S.Hd[tri(kk, kk)] : 1.f;
#pragma unroll
            for (int j = 0; j < kk; j++) {
              const float t = dact ? S.Hd[tri(kk, j)] : 0.f;
              dp = fmaf(t, t, dp);
              if (kk < 16) s0 = fmaf(-h0[j < 16 ? j : 0], t, s0);
              s1 = fmaf(-h1[j], t, s1);
            }
            const float rk = __frsqrt_rn(fmaxf(hkk - dp, 1e-30f));
            if (kk < 16) h0[kk < 16 ? kk : 0] = kk <= l ? s0 * rk : 0.f;
            h1[kk] = (two && kk <= r1) ? s1 * rk : 0.f;
            if (dact) {
              if (kk < 16 && l > kk) S.Hd[tri(l, kk)] = h0[kk < 16 ? kk : 0];
              if (two && r1 > kk) S.Hd[tri(r1, kk)] = h1[kk];
              if (l == 0) S.dinv[kk] = rk;
            }
            WSYNC();
          }
          // L y = -g: the owner of row k publishes y_k, every lane takes it out of its own rows' right-hand sides
          float b0 = dact ? -S.g[l] : 0.f, b1 = (dact && two) ? -S.g[r1] : 0.f;
#pragma unroll
          for (int kk = 0; kk < NV; kk++) {
            if (dact && (kk < 16 ? l == kk : r1 == kk)) S.p[kk] = (kk < 16 ? b0 : b1) * S.dinv[kk];
            WSYNC();
            const float yk = dact ? S.p[kk] : 0.f;
            if (kk < 16) b0 -= (l > kk ? h0[kk < 16 ? kk : 0] : 0.f) * yk;
            b1 -= ((two && r1 > kk) ? h1[kk] : 0.f) * yk;
          }
          // L' x = y, in place: the owner of row k finishes x_k and takes it out of the entries above
#pragma unroll
          for (int kk = NV - 1; kk >= 0; kk--) {
            if (dact && (kk < 16 ? l == kk : r1 == kk)) {
              const float xk = S.p[kk] * S.dinv[kk];
              S.p[kk] = xk;
#pragma unroll
              for (int j = 0; j < kk; j++) S.p[j] -= (kk < 16 ? h0[j < 16 ? j : 0] : h1[j]) * xk;
            }
            WSYNC();
          }
          if (dact) {
            p_own = S.p[6 + l]; xcl = l < 6 ? S.p[l] : 0.f;
            for (int k = 0; k < 6; k++) xc6[k] = S.p[k];
            for (int j = 0; j < NLK; j++) pc4[j] = S.p[6 + 4 * c + j];
          }
        }
}
        V5_TICK(9)
        // ---- (5) exact line search along p
        float Mp_own = 0.f;
#pragma unroll
        for (int j = 0; j < NLK; j++) Mp_own += Mrow[j] * pc4[j];
        const float pMp = gsum(p_own * Mp_own + mck * xcl * xcl);
        const float pMd = gsum(Mp_own * da_own + mck * xcl * dcl);
        const float gp = gsum(g_own * p_own + gcl * xcl);
        if (act && !(gp < 0.f)) act = false;
        {
          const float* wa = xc6 + 3;
#pragma unroll
          for (int k = 0; k < NS; k++) {
            if (!HC && k == 0) { slot_Jx_first(sl[0], xc6, wa, S.p, sl[0].jp, V5_C3C(0)); continue; }
            if (k > 0 && !((used >> k) & 1u)) continue;  // (wave-uniform: nobody's slot k holds a contact)
            if (sl[k].la >= 0) slot_Jx<HC>(sl[k], S, qc, xc6, wa, S.p, sl[k].jp, V5_C3C(k));
          }
        }
        dr.pf = p_own; dr.pl = dr.lims * p_own;
        V5_TICK(10)
        float lo = 0.f, hi = -1.f, alpha = 1.f; bool lsact = act;
#ifdef JH_V5_CENSUS
        int cen_ls = 0, cen_lsw = 0; const bool cen_act = act;
        if (stats && lane == 0) atomicAdd(stats + 320 + __popcll(__ballot(act && l == 0)), 1);
#endif
        for (int ls = 0; ls < LSMAX && __any(lsact); ls++) {
          float d1, d2;
#ifdef JH_V5_CENSUS
          cen_ls += lsact; cen_lsw++;
#endif
          lane_rows_dir<NS>(sl, dr, alpha, &d1, &d2, used);
          d1 = gsum(d1) + pMd + alpha * pMp; d2 = gsum(d2) + pMp;
          {  // safeguarded Newton step on the slope, as selects (round 6: the nested branches were a dozen exec-mask instructions per evaluation; the same arithmetic)
            const bool upd = lsact & !(fabsf(d1) <= lstol * fabsf(gp)), neg = d1 < 0.f;
            lo = (upd & neg) ? alpha : lo; hi = (upd & !neg) ? alpha : hi;
            float nx = alpha - d1 * __builtin_amdgcn_rcpf(d2);  // (v_rcp_f32, 1 ulp: the correctly rounded division is 10 instructions per evaluation)
            const bool out_lo = nx <= lo, out_hi = nx >= hi;
            float dbl = 2.f * alpha, mid_ = 0.5f * (lo + hi); asm volatile("" : "+v"(dbl), "+v"(mid_));  // (both computed: selects, not branches)
            nx = hi < 0.f ? (out_lo ? dbl : nx) : ((out_lo | out_hi) ? mid_ : nx);
            alpha = upd ? nx : alpha; lsact = upd;
          }
        }
#ifdef JH_V5_CENSUS
        if (stats) { if (l == 0 && live && cen_act) atomicAdd(stats + 256 + min(cen_ls, 31), 1); if (lane == 0) atomicAdd(stats + 288 + min(cen_lsw, 31), 1); }
#endif
        V5_TICK(11)
        // ---- (6) step
        if (act) {
          a_own += alpha * p_own; ac_own += alpha * xcl;
#pragma unroll
          for (int k = 0; k < NS; k++) if (sl[k].la >= 0) for (int rw = 0; rw < 3; rw++) sl[k].jar[rw] += alpha * sl[k].jp[rw];
          dr.jf += alpha * dr.pf; dr.jl += alpha * dr.pl;
          if (-gp * alpha <= tol * tol * fmaxf(snorm, 1e-12f)) act = false;
        }
        WSYNC();
        V5_TICK(12)
      }
      };
      // (the rare slot-count copy instantiates the dense-capable loop only -- it serves rollouts without a dense row as well: three copies of the loop instead of four, and
      // the common one came out 0.9 % faster for it)
      if constexpr (HC && NS > NSLOT) newton_loop(std::true_type{});
      else if constexpr (HC && NS == NSLOT) { if (__any(dense_row)) newton_loop(std::true_type{}); else newton_loop(std::false_type{}); }
      else newton_loop(std::false_type{});
      if (l == 0) { n_iters += iters_this; n_maxed += (iters_this >= cap); }
    }
    };
    if (__builtin_expect_with_probability(NSBIG > NSLOT && __any(S.ncon > 16 * NSLOT), 0, BIGPROB)) {
      if (NOVF > 0 && __any(S.ncon > NCP)) __threadfence();  // the overflow rows were written with plain global stores by other lanes of this wave
      solve_step(std::integral_constant<int, NSBIG>{}, std::integral_constant<bool, SELF>{});
    } else {
      // A wave-step in which no rollout has a candidate pair off the cube (two thirds of them on the headline workload) has cube contacts only: it takes the copy of the solver
      // compiled without the code for the hand's own contacts (link on side A, chain-coupling blocks, staged elimination, dense direction) -- the same expressions for what
      // remains, fewer live values around them: 61.1 -> 59.4 ms.  The same contacts through the hand-capable copy cost 14 % more (48.5 against 42.5 ms with the hand's broad
      // phase switched off) for the registers its extra paths hold.  The two copies must give the same bits for a cube contact (a rollout's result may not depend on its
      // wave-mates: tests/test_gpu_leap.py permutes them): with -ffp-contract=fast they do not -- the backend fuses a product into an add only when the product has no other
      // use, and the hand paths are such uses -- so this file is built with -ffp-contract=on (fusion within a source expression only: +0.7 % on its own, jh_engine_v5.flags).
      if (SELF && !__any(hand_hits)) solve_step(std::integral_constant<int, NSLOT>{}, std::false_type{});
      else solve_step(std::integral_constant<int, NSLOT>{}, std::integral_constant<bool, SELF>{});
    }
#ifdef JH_V5_CENSUS
    if (stats) { if (l == 0 && live) atomicAdd(stats + 192 + min(iters_this, 31), 1); if (lane == 0) atomicAdd(stats + 224 + min(n_wave_iters - wave_it0, 31), 1); }
#endif
    // ================================================================ implicitfast integration: (M + h diag(d + kv)) qacc = fs + M (a - a0)
    {
      S.ws[6 + l] = a_own; if (l < 6) { S.acn[l] = ac_own; if (l < 3) S.ws[l] = ac_own; }  // (rotational part: world here; body frame below)
      q = S.pk_q[l]; qd = S.qv[6 + l]; fs_own = S.pk_fs[l];  // (own entries: no other lane wrote them)
      const float da_own = a_own - a0_own;
      float rhs_own = fs_own, x4[NLK], L[10];
#pragma unroll
      for (int j = 0; j < NLK; j++) rhs_own += Mrow[j] * quad_get(da_own, j);
#pragma unroll
      for (int j = 0; j < NLK; j++) x4[j] = quad_get(rhs_own, j);
      for (int k = 0; k < 10; k++) L[k] = S.Mbb[c][k];
      const float hdk = h * (lc[LC_DAMP] + lc[LC_KVD]);
#pragma unroll
      for (int j = 0; j < NLK; j++) L[tri(j, j)] += quad_get(hdk, j);
      float inv4[4]; chol4(L, inv4); fwd4(L, inv4, x4); bwd4(L, inv4, x4);
      const float qacc = sel4(x4, s);
      qd = fmaf(h, qacc, qd); q = fmaf(h, qd, q);
      WSYNC();
      for (int k = 0; k < 6; k++) vc[k] = S.qv[k];
      for (int k = 0; k < 4; k++) qc[3 + k] = S.pk_cq[k];
      if (!MATERIALIZE) acc = S.pk_acc;
      {  // the constrained rotational acceleration back in the body frame (MuJoCo's free-joint convention): integrated, and kept as the next step's warm start
        const float aw[3] = {S.acn[3], S.acn[4], S.acn[5]}; float ab[3]; mulMTV(ab, S.xR[0], aw);
        for (int k = 0; k < 3; k++) { vc[k] = fmaf(h, S.acn[k], vc[k]); vc[3 + k] = fmaf(h, ab[k], vc[3 + k]); }
        if (l < 3) S.ws[3 + l] = l == 0 ? ab[0] : (l == 1 ? ab[1] : ab[2]);
      }
      for (int k = 0; k < 3; k++) qc[k] = fmaf(h, vc[k], qc[k]);
      float wn = sqrtf(vc[3] * vc[3] + vc[4] * vc[4] + vc[5] * vc[5]), ang = wn * h;
      if (ang > 0.f) {
        float sn, cs; sincosf(0.5f * ang, &sn, &cs); float kk = sn / wn;
        float dq[4] = {cs, vc[3] * kk, vc[4] * kk, vc[5] * kk}, *qq = qc + 3;
        float r0 = qq[0] * dq[0] - qq[1] * dq[1] - qq[2] * dq[2] - qq[3] * dq[3];
        float r1 = qq[0] * dq[1] + qq[1] * dq[0] + qq[2] * dq[3] - qq[3] * dq[2];
        float r2 = qq[0] * dq[2] - qq[1] * dq[3] + qq[2] * dq[0] + qq[3] * dq[1];
        float r3 = qq[0] * dq[3] + qq[1] * dq[2] - qq[2] * dq[1] + qq[3] * dq[0];
        qq[0] = r0; qq[1] = r1; qq[2] = r2; qq[3] = r3;
      }
      float nn = rsqrtf(qc[3] * qc[3] + qc[4] * qc[4] + qc[5] * qc[5] + qc[6] * qc[6]);
      qc[3] *= nn; qc[4] *= nn; qc[5] *= nn; qc[6] *= nn;
    }
    V5_TICK(7)
    if (MATERIALIZE) {
      if (states && live) {
        float* o = states + ((size_t)nc * H + hh) * NX;
        o[7 + l] = q; o[NQ + 6 + l] = qd;
        if (l < 7) o[l] = qc[l];
        if (l < 6) o[NQ + l] = vc[l];
      }
    } else acc += leap_step_cost(sTp, qc);
    WSYNC();
  }
  if constexpr (PERSIST) {  // a missed hand-off: that was the group up to the slice's first step -- once more round the loop for the slice, nothing flushed
    again = __builtin_amdgcn_readfirstlane(sUnit[4 * wv]) < __builtin_amdgcn_readfirstlane(sUnit[4 * wv + 2]);
    if (again) { if (lane == 0 && stats_) atomicAdd(stats_ + JH_STAT_RECOMPUTED, 1); continue; }
  }
  int usteps = H; bool last = true;  // the steps this unit ran (and counts); whether it ends the rollouts
  if constexpr (PERSIST) { const int h0 = __builtin_amdgcn_readfirstlane(sUnit[4 * wv + 1]), h1 = __builtin_amdgcn_readfirstlane(sUnit[4 * wv + 2]); usteps = h1 - h0; last = h1 >= H; unit = __builtin_amdgcn_readfirstlane(sUnit[4 * wv + 3]); }
#ifdef JH_V5_COUNT
  if (stats) { if (lane == 0) { atomicAdd(stats + 24, cnt_dense); atomicAdd(stats + 25, cnt_it); atomicAdd(stats + 26, cnt_l2); atomicAdd(stats + 28, usteps); } if (l == 0 && live) { atomicAdd(stats + 27, cnt_bp); atomicAdd(stats + 29, cnt_hh); for (int k = 0; k < 4; k++) atomicAdd(stats + 30 + k, cnt_cls[k]); } }
#endif
#ifdef JH_V5_TICKS
  if (lane == 0 && stats) { for (int k = 0; k < 8; k++) atomicAdd((unsigned long long*)(stats + 4) + k, (unsigned long long)cyc[k]);
                            for (int k = 0; k < 16; k++) atomicAdd((unsigned long long*)(stats + 384) + k, (unsigned long long)cyc[k]); }
#endif
  if (!MATERIALIZE && live && l == 0 && last) costs[n] = acc / (float)H;
  if (stats && live && l == 0) { if (n_maxed) atomicAdd(stats + JH_STAT_ITER_CAP, n_maxed); atomicAdd(stats + JH_STAT_ITERS, n_iters); atomicAdd(stats + JH_STAT_STEPS, usteps); }
  if (stats && lane == 0 && live) { atomicAdd(stats + JH_STAT_WAVE_ITERS, n_wave_iters); atomicAdd(stats + JH_STAT_WAVE_STEPS, usteps); }
  if constexpr (PERSIST) if (!last) {  // park the state for the next slice: the rows, a device-scope release by the whole wave, then the unit's flag
    float* pk = park + (size_t)unit * PARK_F;
    float pv = l == 13 ? acc : 0.f;
    for (int k = 0; k < 7; k++) if (l == k) pv = qc[k];
    for (int k = 0; k < 6; k++) if (l == 7 + k) pv = vc[k];
    PARK_ST(pk + lane, q); PARK_ST(pk + 64 + lane, qd); PARK_ST(pk + 128 + lane, S.ws[6 + l]); PARK_ST(pk + 192 + lane, pv); PARK_ST(pk + 256 + lane, l < 6 ? S.ws[l] : 0.f);
    __threadfence();
    if (lane == 0) __hip_atomic_store(pflags + unit, 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
  }
#ifdef JH_V5_WAVESTAMP
  if (lane == 0 && g_wavestamp && (PERSIST ? unit : grp) < g_wavestamp_cap) {  // (a row per queue unit: ticket t is slice t / groups of group t % groups)
    unsigned long long* w = g_wavestamp + (size_t)(PERSIST ? unit : grp) * 6;
    w[0] = ((unsigned long long)blockIdx.x << 32) | ((unsigned long long)wv << 8) | (__smid() & 0xff); w[1] = ws_entry; w[2] = ws_staged; w[3] = ws_start; w[4] = wall_clock64(); w[5] = 1;
  }
#endif
  if constexpr (!PERSIST) break;
  else {  // the next ticket: one returning device-scope atomic per group (a vector atomic of lane 0, broadcast to the wave)
    int t = 0;
    if (lane == 0) t = (int)atomicAdd(head, 1u);
    unit = (int)(gridDim.x * WPB) + __builtin_amdgcn_readfirstlane(t);
  }
  }
}

bool model_is_leap(const jh_model* m) {
  const HostImage& im = m->image;
  return im.fits && m->kind == JH_TASK_LEAP_CUBE && m->nq == 23 && m->nv == 22 && m->nu == 16 && (m->ns == NS || (m->ns == NS_CALTECH && im.oRef > 0)) &&
         im.v.NM == 17 && im.v.NBLK == 4 && im.oLane > 0 && im.v.NG <= MAXG && im.LGM <= MAXLG && im.NBP <= MAXBP
         && m->h_f[HF_CINERTIA] == m->h_f[HF_CINERTIA + 1] && m->h_f[HF_CINERTIA] == m->h_f[HF_CINERTIA + 2]  // isotropic cube inertia: the solver works on the rotation in the world frame
         ;
}

int device_cus(const jh_model* m) {  // (per call, of the model's device: a process may drive several)
  int v = 0;
  return (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, m->device) == hipSuccess && v > 0) ? v : 256;
}

// The build's acceptance test: JH_OK, or the status with the error set under the caller's name (`who` null: no message).
int leap_refusal(const jh_model* m, const char* who) {
  if (!model_is_leap(m)) { if (who) jh_set_error("%s: the cooperative engine kernel is instantiated for leap_cube only", who); return JH_ERR_UNSUPPORTED; }
  if ((m->cylinders > 0) != (JH_V5_CYL != 0)) { if (who) jh_set_error("%s: an image with cylinder geoms runs on the cylinder build of the leap kernel and no other image does (%d cylinders)", who, m->cylinders); return JH_ERR_UNSUPPORTED; }
  return JH_OK;
}
bool accepts(const jh_model* m) { return leap_refusal(m, nullptr) == JH_OK; }

// k_leap_v5's arguments: the fused launch's record `a` (materialise mode: x0, N, H, the rest null / 0) and what stands beside it.  What a launch shape does not use stays null / 0.
struct LeapArgs {
  const jh_rollout_args& a; const float* gF; const int* gI; int* stats; int dshift, grid;  // grid: not an argument -- the workgroups of a problem on the static grid
  int x0_batched = 0; const float* controls = nullptr; float *states = nullptr, *sensors = nullptr;  // materialise mode
  float* ovf = nullptr; unsigned *head = nullptr, *pflags = nullptr; int slices = 0; BatchBounds sb = {};  // (the plant axis behind the eight words goes to the batched instantiations alone)
  long long batch_blk = 0, batch_noise = 0, batch_image = 0;
};

// What every launcher starts with: the latency shift chosen from the `rollouts` of the whole launch and the static grid for a problem's N.
LeapArgs leap_args(const jh_model* m, const jh_rollout_args& a, const float* gF, const int* gI, int rollouts) {
  const int dshift = jh_latency_shift(rollouts, RPW), per_block = (RPW >> dshift) * WAVES_PER_BLOCK;
  return {a, gF, gI, m->d_stats, dshift, (a.N + per_block - 1) / per_block};
}

// one row per rollout for the contacts above the LDS pool
size_t ovf_bytes(size_t rows) { return NOVF > 0 ? rows * NOVF * POOL_F * sizeof(float) : 0; }

template <bool MATERIALIZE, bool SELF, bool PERSIST = false, bool BATCH = false>
void launch(const LeapArgs& k, dim3 grid, hipStream_t st) {
  const jh_rollout_args& a = k.a;
  hipLaunchKernelGGL((k_leap_v5<MATERIALIZE, WAVES_PER_BLOCK, SELF, PERSIST, BATCH>), grid, dim3(WAVE * WAVES_PER_BLOCK), 0, st, k.gF, k.gI, a.x0, k.x0_batched, a.nominal, a.noise, a.ldn,
                     a.sigma, a.W, a.lohi, a.tp, a.N, a.n_offset, a.H, a.K, a.costs, a.knots_out, k.controls, k.states, k.sensors, k.stats, k.dshift, a.trace, k.ovf, k.head,
                     k.batch_blk, k.batch_noise, k.batch_image, k.pflags, k.slices, static_cast<const std::conditional_t<BATCH, BatchBounds, SliceBounds>&>(k.sb));
}

bool hand_contacts(const jh_model* m) { return m->self_collision && m->image.fits && m->image.NBP > 0; }  // the SELF instantiations: the hand's own contacts are on and the image has body pairs

}  // namespace

#ifndef JH_V5_NAME
#define JH_V5_NAME(f) f
#endif
#ifdef JH_V5_WAVESTAMP
extern "C" int JH_V5_NAME(jh_v5_wavestamp_buffer)(unsigned long long* buf, int groups) {  // diagnostic builds: where the kernel stores its stamps (nullptr: nowhere)
  JH_HIP(hipMemcpyToSymbol(HIP_SYMBOL(g_wavestamp), &buf, sizeof(buf)));
  JH_HIP(hipMemcpyToSymbol(HIP_SYMBOL(g_wavestamp_cap), &groups, sizeof(groups)));
  return JH_OK;
}
#endif
static int rollout_cost(const jh_model* m, const jh_rollout_args& a, hipStream_t st) {
  if (int rc = leap_refusal(m, "rollout_cost")) return rc;
  const int N = a.N, H = a.H;
  LeapArgs k = leap_args(m, a, m->d_f, m->d_i, N);
  // Launch shape (jh_model_set_rollout_schedule).  A launch with more groups of four rollouts than the GPU holds waves of this kernel (two workgroups per CU) runs one workgroup
  // per resident slot and lets the waves draw their groups from a queue; one that fits at once, and every latency-mode launch, keeps one group per wave of the grid.
  bool persist = k.dshift == 0 && m->rollout_schedule != 1; int slots = 0;
  if (persist) { slots = 2 * device_cus(m); persist = m->rollout_schedule == 2 || k.grid > slots; }
  // Horizon slices (jh_model_set_rollout_slices): the queue's units are (group, slice) where the queue runs and the launch has at least two groups per wave slot -- dependent
  // units are then so many tickets apart that a slice's predecessor has as good as always parked its state in time -- or wherever the queue runs if a number is forced.
  const int ngroups = (N + RPW - 1) / RPW;
  // The slices' first steps come from the model's explicit schedule (jh_model_set_rollout_slice_bounds; bounds at or behind H are dropped, so a schedule holds for any horizon),
  // from a forced number of equal slices, or from the automatic rule (jh_rollout_slice_schedule: a taper where the queue is deep, equal slices from two groups per wave slot).
  // Equal slices run on the kernel's own division, as they did before there was a table; any other schedule goes to the kernel as its table of bounds.
  int slices = 1, bounds[JH_MAX_SLICE_BOUNDS], nb = 0; bool table = false;
  if (persist) {
    if (m->rollout_nbounds > 0) { for (int i = 0; i < m->rollout_nbounds; i++) if (m->rollout_bounds[i] < H) bounds[nb++] = m->rollout_bounds[i]; slices = nb + 1; }
    else if (m->rollout_slices > 0) slices = m->rollout_slices;
    else { nb = jh_rollout_slice_schedule(H, ngroups, slots * WAVES_PER_BLOCK, bounds, JH_MAX_SLICE_BOUNDS); slices = nb + 1; }
    if (slices > H) slices = H;
    if (slices < 1 || (long long)slices * ngroups > 0x7fffffffll) slices = 1;
    for (int i = 0; i < nb && slices == nb + 1; i++) table = table || bounds[i] != (i + 1) * H / slices;
    if (table && (slices > MAX_BOUND_SLICES || H > 0xffff)) { slices = 1; table = false; }  // (what the table cannot hold: never reached through the setters and the rule)
  }
  // Stream-ordered scratch of the launch, no state on the model handle (two streams may run one model): the queue's head word in a 16-byte block, the flag words of the
  // slices (one per unit, padded to 16 bytes) -- both zeroed in front of every launch that uses them --, the parked rows of the slices, then one row per rollout for the
  // contacts above the LDS pool and, under slices, one more per rollout row of every wave slot for a pass that recomputes a missed hand-off.  A sliced request the pool
  // refuses is asked again for whole groups (the parked rows are the bulk of it) before the launch gives the queue up.
  int qgrid = k.grid;  // the queue's grid
  if (persist) { if (qgrid > slots) qgrid = slots; if (m->rollout_max_workgroups > 0 && qgrid > m->rollout_max_workgroups) qgrid = m->rollout_max_workgroups; }  // (the cap: a test hook, few waves and many tickets)
  size_t flag_words = 0, queue_bytes = 0, ovf_b = 0;
  float* scratch = nullptr; unsigned* head = nullptr;
  for (;;) {
    flag_words = slices > 1 ? (((size_t)slices * ngroups + 3) & ~(size_t)3) : 0;
    const size_t park_floats = slices > 1 ? (size_t)(slices - 1) * ngroups * PARK_F : 0, own_rows = slices > 1 ? (size_t)qgrid * WAVES_PER_BLOCK * RPW : 0;
    queue_bytes = persist ? 16 + (flag_words + park_floats) * sizeof(float) : 0;
    ovf_b = ovf_bytes((size_t)N + own_rows);
    if (ovf_b > 0 || persist) scratch = jh_launch_scratch(m, ovf_b + queue_bytes, st, ovf_b > 0 && slices == 1);  // (nullptr: the LDS capacity alone, drops and the fallback counted -- and the static shape)
    if (scratch || slices == 1) break;
    slices = 1; table = false;
  }
  if (scratch && persist && hipMemsetAsync(scratch, 0, 16 + flag_words * sizeof(unsigned), st) != hipSuccess) { (void)hipGetLastError(); persist = false; }
  if (!scratch) persist = false;
  if (persist) { head = (unsigned*)scratch; k.grid = qgrid; } else { slices = 1; table = false; }
  if (table) for (int i = 0; i < MAX_BOUND_SLICES; i++) k.sb.w[i >> 1] |= (unsigned)(i < nb ? bounds[i] : H) << ((i & 1) << 4);
  jh_model_note_slice_bounds(m, slices, H, table ? bounds : nullptr);
  if (scratch && ovf_b > 0) k.ovf = scratch + (head ? queue_bytes / sizeof(float) : 0);
  __atomic_store_n(&m->last_rollout_slices, persist ? slices : 0, __ATOMIC_RELAXED);
  k.head = head; k.pflags = head ? head + 4 : nullptr; k.slices = slices | ((m->rollout_slice_flags & 1) << 8) | (table ? 0x200 : 0);
  if (hand_contacts(m)) { if (persist) launch<false, true, true>(k, dim3(k.grid), st); else launch<false, true, false>(k, dim3(k.grid), st); }
  else { if (persist) launch<false, false, true>(k, dim3(k.grid), st); else launch<false, false, false>(k, dim3(k.grid), st); }
  return jh_launch_done(scratch, st);
}

static int materialize(const jh_model* m, const float* x0, int x0_batched, const float* controls, int N, int H, float* states, float* sensors, hipStream_t st) {
  if (int rc = leap_refusal(m, "rollout_materialize")) return rc;
  jh_rollout_args a = {};
  a.x0 = x0; a.N = N; a.H = H;
  LeapArgs k = leap_args(m, a, m->d_f, m->d_i, N);
  k.x0_batched = x0_batched; k.controls = controls; k.states = states; k.sensors = sensors;
  if (const size_t b = ovf_bytes(N)) k.ovf = jh_launch_scratch(m, b, st);  // stream-ordered allocation, no state on the model handle (nullptr: the LDS capacity alone, drops and the fallback counted)
  if (hand_contacts(m)) launch<true, true>(k, dim3(k.grid), st);
  else launch<true, false>(k, dim3(k.grid), st);
  return jh_launch_done(k.ovf, st);
}

// (Defined last in the file: the batched instantiations are emitted behind every other kernel and shift none of them in the code object.)
// B problems in one launch (jh_plan_step_batch): the static grid with the problem in its second dimension.  The record is problem 0's; `blk_stride` / `noise_stride` floats
// lead to the next problem's, and `image_stride` floats from `images`, problem 0's float section, to the next problem's (m->d_f and 0 where the problems share the model;
// a model set's members passed the row's `accepts` one by one when the set was made).  The latency shift is chosen from B * N, the rollouts of the launch (the bits do
// not depend on it), and there is no queue.
static int rollout_cost_batch(const jh_model* m, const jh_rollout_args& a, const jh_rollout_batch& s, hipStream_t st) {
  if (int rc = leap_refusal(m, "plan_step_batch")) return rc;
  const long long rollouts = (long long)s.C * s.B * a.N;  // (s.C: the controller axis of jh_plan_step_ensemble_batch, 1 everywhere else)
  JH_REQUIRE(s.C >= 1 && s.C <= 65535 && rollouts <= 0x7fffffffll, "plan_step_batch: B * N = %lld rollouts exceed one launch", rollouts);
  LeapArgs k = leap_args(m, a, s.images, s.ints, (int)rollouts);
  k.batch_blk = s.blk_stride; k.batch_noise = s.noise_stride; k.batch_image = s.image_stride;
  set_axis_stride(k.sb, 0, s.blk_stride_c); set_axis_stride(k.sb, 1, s.noise_stride_c); set_axis_stride(k.sb, 2, s.image_stride_c);
  k.sb.plants = s.plants;
  if (const size_t b = ovf_bytes((size_t)rollouts)) k.ovf = jh_launch_scratch(m, b, st);  // (every problem's rows; nullptr: the LDS capacity alone, drops and the fallback counted)
  if (hand_contacts(m)) launch<false, true, false, true>(k, dim3(k.grid, s.B, s.C), st);
  else launch<false, false, false, true>(k, dim3(k.grid, s.B, s.C), st);
  return jh_launch_done(k.ovf, st);
}

// (Behind the fused batched launch for the same reason.)  Materialise mode on a plant axis (jh_rollout_materialize_plants): s.B blocks of n rollouts on the grid (groups of
// a block, s.B), block g on image s.plants[g] of s.images and on the one int section s.ints.  x0 is one state, or one per row of the s.B * n; the controls are a block's own
// n rows, or rows [0, n) for every block.  The latency shift is chosen from s.B * n, the rollouts of the launch (the bits do not depend on it); a block's rows never share
// a wave with another block's, and a dead row of a block's last wave recomputes that block's last rollout.
static int materialize_plants(const jh_model* m, const jh_rollout_batch& s, const float* x0, int x0_batched, const float* controls, int controls_shared, int n, int H, float* states,
                              float* sensors, hipStream_t st) {
  if (int rc = leap_refusal(m, "rollout_materialize_plants")) return rc;
  const long long rollouts = (long long)s.B * n;
  JH_REQUIRE(rollouts <= 0x7fffffffll, "rollout_materialize_plants: G * n = %lld rollouts exceed one launch", rollouts);
  jh_rollout_args a = {};
  a.x0 = x0; a.N = n; a.H = H;
  LeapArgs k = leap_args(m, a, s.images, s.ints, (int)rollouts);
  k.x0_batched = x0_batched; k.controls = controls; k.states = states; k.sensors = sensors;
  k.batch_blk = controls_shared ? 0 : (long long)n * H * NU; k.batch_noise = x0_batched ? (long long)n * NX : 0; k.batch_image = s.image_stride;
  k.sb.plants = s.plants;
  if (const size_t b = ovf_bytes((size_t)rollouts)) k.ovf = jh_launch_scratch(m, b, st);  // (every block's rows; nullptr: the LDS capacity alone, drops and the fallback counted)
  if (hand_contacts(m)) launch<true, true, false, true>(k, dim3(k.grid, s.B), st);
  else launch<true, false, false, true>(k, dim3(k.grid, s.B), st);
  return jh_launch_done(k.ovf, st);
}

// This build's row of the table (jh_internal.h); `accepts` is what the launchers above ask of a model, for a caller that must know in advance (jh_model_set_create: every
// member of a set, on its own floats).  Host pass only: a const object with a constant initialiser would be emitted into the code object as well.
// No bound of its own on K: the kernel reads its knots from memory every step, no on-chip staging.  The trace: trace_cube, trace_{if,mf,rf,th}_tip, the five framepos
// sensors behind the 16 joint positions of leap_cube.xml's NS sensors (the kernel writes them for that sensor list alone).
#ifndef __HIP_DEVICE_COMPILE__
const jh_engine_build JH_V5_NAME(jh_engine5_build) = {JH_V5_CYL ? "leap, cylinders" : NCAP > 48 ? "leap, 64 contacts" : "leap, 48 contacts", accepts, rollout_cost, rollout_cost_batch, materialize, NCAP, materialize_plants,
                                                      nullptr, [](const jh_model* m) { return m->ns == NS ? jh_trace_layout{16, 15, 0} : jh_trace_layout{}; }};
#endif
