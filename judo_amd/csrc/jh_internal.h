// jh_internal.h -- shared definitions of libjudo_amd.so (gfx950 only; no other backend exists).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "jh_image.h"  // (the articulated models' image: layout, view, host readers)
#include "judo_amd.h"
#include "judo_amd_xcheck.h"  // (the test-build hooks: the cross-check kernel generations register through them)

#define JH_BLOB_MAGIC 0x314D484Au /* "JHM1" */
#define JH_BLOB_VERSION 1u
#define JH_NSTATS 512
// Host-side blob header produced by judo_amd/models.py::pack_model (little-endian, 64 bytes):
struct jh_blob_header {
  uint32_t magic, version, kind, nq, nv, nu, ns, ntaskparam, nfloat, nint;
  uint32_t reserved[6];
};

constexpr int JH_MAX_SLICE_BOUNDS = 15;  // an explicit schedule has at most 16 slices: the kernel's table of bounds (jh_engine_v5.hip)

struct jh_model {
  int device, kind, nq, nv, nu, ns, ntaskparam;
  size_t nf, ni;
  float* d_f;  // device copy of the float section
  int* d_i;    // device copy of the int section
  int kernel_gen;  // articulated engine kernel: 3 = cooperative 16-lanes-per-rollout, two waves per SIMD (leap_cube: v5; fr3_pick: v6, matrix-free contact Jacobian), 2 = cooperative, one wave per SIMD (leap_cube: v2, fr3_pick: v3), 1 = one lane per rollout
  int contact_capacity;  // leap_cube generation 3: 48 (all in LDS, jh_engine_v5.hip) or 64 (jh_engine_v5_cap64.hip); jh_model_set_contact_capacity
  int cylinders;  // leap_cube family: cylinder geoms in the image (caltech_leap_cube packed with fingertips="cylinder"); > 0 selects the cylinder build (jh_engine_v5_cyl.hip: generation 3, 64 contacts) and nothing else runs such an image
  int arm_pairs;  // fr3_pick: candidate pairs of the image between two arm bodies other than the two fingers, or of a box on the arm against a capsule on the arm or the static base (engine_model.pack_engine_model on a description with "self_collision"); > 0 selects the self-collision build (jh_engine_v6_self.hip: generation 3) and nothing else runs such an image
  int self_collision;  // leap_cube on jh_engine_v5.hip: model the hand's own contacts (finger-finger, finger-palm) as MuJoCo does; 0 = the cube's contacts only
  int rollout_schedule;  // leap_cube generation 3, fused launches: 0 = persistent waves on a queue of rollout groups where the launch exceeds the GPU's wave slots (the default), 1 = always the static grid, 2 = the queue wherever the kernel has it (jh_model_set_rollout_schedule)
  int rollout_slices = 0, rollout_max_workgroups = 0, rollout_slice_flags = 0;  // the queue's horizon slices (jh_model_set_rollout_slices): 0 = automatic or 1..64 forced; a cap on the queue's grid (0: the resident slots); bit 0: every hand-off counts as missed
  int rollout_bounds[JH_MAX_SLICE_BOUNDS] = {}, rollout_nbounds = 0;  // an explicit schedule of slices (jh_model_set_rollout_slice_bounds): the first steps of slices 1 .. n, strictly increasing; n = 0: none.  The later call of the two setters decides
  mutable int last_rollout_bounds[63] = {}, last_rollout_nbounds = 0;  // the first steps of slices 1 .. S - 1 of that launch (jh_model_last_rollout_slice_bounds); __atomic builtins
  mutable int last_rollout_slices = 0;  // what the model's last fused leap launch ran: 0 = the static grid, 1 = the queue of groups, S > 1 = the queue of S slices per group (jh_model_last_rollout_slices); __atomic builtins, as ovf_fallbacks
  int plan_step_launches;  // closed-form models' plan step: 0 = one launch where it fits (the default), 1 = always one launch, 2 = always two (jh_model_set_plan_step_launches)
  mutable int one_launch_steps = 0;  // plan steps that ran as one launch (jh_model_stats out[7]); __atomic builtins, as ovf_fallbacks
  mutable int ovf_fallbacks = 0;  // launches that ran without their overflow rows (jh_launch_scratch); updated with __atomic builtins: a planner thread may launch while another polls jh_model_stats
  int* d_stats;  // JH_NSTATS diagnostic counters: the JH_STAT_* words below; the rest: diagnostic builds
  std::vector<float> h_f;
  std::vector<int> h_i;
  jh_eng::HostImage image;  // the articulated kinds: the view of h_f / h_i and whether it fits them and the blob header's dimensions (jh_model_create, once); the launchers' acceptance tests ask it first
};

void jh_set_error(const char* fmt, ...);
// The leap launcher's record of the slices it ran (jh_api.hip): `bounds` null = `slices` equal ones of a horizon H.
void jh_model_note_slice_bounds(const jh_model* m, int slices, int H, const int* bounds);

// Per-launch scratch of the cooperative kernels (the contacts above the LDS pool, one row per rollout): a stream-ordered allocation from the default pool of the MODEL's
// device (not of whatever device is current in the calling thread).  nullptr when the pool refuses: the kernel then holds what its LDS pool holds, the drops are
// counted, and the launch is counted in `ovf_fallbacks` (jh_model_stats out[6]) so that the lower capacity does not go unnoticed.  `overflow_rows` = false: the block
// holds no overflow rows (the leap kernel's queue head alone), and a refusal costs no capacity and is not counted.
inline float* jh_launch_scratch(const jh_model* m, size_t bytes, hipStream_t st, bool overflow_rows = true) {
  hipMemPool_t pool = nullptr; void* p = nullptr;
  if (hipDeviceGetDefaultMemPool(&pool, m->device) == hipSuccess && pool && hipMallocFromPoolAsync(&p, bytes, pool, st) == hipSuccess) return (float*)p;
  (void)hipGetLastError();
  if (!overflow_rows) return nullptr;
  if (__atomic_fetch_add(&m->ovf_fallbacks, 1, __ATOMIC_RELAXED) == 0)  // the first fallback of a model is also logged: the lower capacity must not depend on somebody polling the counter
    fprintf(stderr, "judo_amd: no stream-ordered scratch for the contacts above the LDS pool (%zu bytes): this launch runs with the LDS capacity alone; see jh_model_stats out[6]\n", bytes);
  return nullptr;
}

#define JH_HIP(call)                                                                      \
  do {                                                                                    \
    hipError_t e__ = (call);                                                              \
    if (e__ != hipSuccess) {                                                              \
      jh_set_error("%s failed: %s (%s:%d)", #call, hipGetErrorString(e__), __FILE__, __LINE__); \
      return JH_ERR_HIP;                                                                  \
    }                                                                                     \
  } while (0)

// end of a cooperative launcher: the launch's error is read FIRST, the stream-ordered overflow block is freed whether the launch succeeded or not, then the error is reported
inline int jh_launch_done(float* ovf, hipStream_t st) {
  const hipError_t e = hipGetLastError();
  const hipError_t f = ovf ? hipFreeAsync(ovf, st) : hipSuccess;
  if (e != hipSuccess) { jh_set_error("kernel launch failed: %s", hipGetErrorString(e)); return JH_ERR_HIP; }
  if (f != hipSuccess) { jh_set_error("hipFreeAsync failed: %s", hipGetErrorString(f)); return JH_ERR_HIP; }
  return JH_OK;
}

#define JH_REQUIRE(cond, ...)    \
  do {                           \
    if (!(cond)) {               \
      jh_set_error(__VA_ARGS__); \
      return JH_ERR_INVALID;     \
    }                            \
  } while (0)

// ---- float-section layouts of the two closed-form models (written by judo_amd/models.py) -------------------
// cartpole (judo/models/xml/cartpole.xml): 2 DoF, contacts disabled, Euler + implicit joint damping
enum {
  CP_DT = 0, CP_G, CP_MCART, CP_MPOLE, CP_L, CP_IPOLE, CP_DAMP_X, CP_DAMP_TH, CP_KP, CP_KV, CP_CTRL_LO, CP_CTRL_HI, CP_CTRL_LIMITED,
  CP_FRC_LO, CP_FRC_HI, CP_FRC_LIMITED, CP_X_LO, CP_X_HI, CP_X_LIMITED, CP_LIM_K, CP_LIM_B, CP_SOLIMP0, CP_SOLIMP1, CP_SOLIMP2,
  CP_SOLIMP3, CP_SOLIMP4, CP_INVW_X, CP_TIP, CP_NPARAM
};
// cylinder_push (judo/models/xml/cylinder_push.xml): 4 slide DoF, one circle-circle contact, Euler + implicit damping
enum {
  CY_DT = 0, CY_MP, CY_MC, CY_DAMP_P, CY_DAMP_C, CY_KP, CY_KV, CY_CTRL_LO, CY_CTRL_HI, CY_CTRL_LIMITED, CY_FRC_LO, CY_FRC_HI,
  CY_FRC_LIMITED, CY_RSUM, CY_CON_K, CY_CON_B, CY_SOLIMP0, CY_SOLIMP1, CY_SOLIMP2, CY_SOLIMP3, CY_SOLIMP4, CY_TRAN, CY_MU, CY_SITE_Z,
  CY_MARGIN, CY_NPARAM
};

// ---- launchers implemented per translation unit ------------------------------------------------------------
// One fused launch (rollouts + cost): what jh_rollout_cost_traced receives after the model.  Filled once by the entry point (or by the plan step, from its packed block's
// offsets) and passed by reference to the launcher.
struct jh_rollout_args {
  const float *x0, *nominal, *noise; int ldn;
  const float *sigma, *W, *lohi, *tp; int phase, N, n_offset, H, K;
  float *costs, *knots_out, *trace;
};
// The plant axis of a batched rollout launch, a kernel argument of the batched rollout kernels and of no other (jh_engine_v5.hip: BATCH; jh_simple.hip: the two *_batch
// kernels): what turns the problems of blockIdx.y into slices of one problem's rollouts, each on a plant of a model set (jh_plan_step_randomized).
//  - n_stride: problem b's rollouts are global rollouts n_offset + b * n_stride + local index.  Only global rollout 0 is the noise-free nominal, so with a stride the
//    first rollout of every later problem keeps its noise.  0: every problem's local rollout 0 is its nominal, the independent problems of jh_plan_step_batch.
//  - the table: problem b reads image plant[b] of the set, a byte per problem packed four to a word, if `mapped`; image b otherwise (the identity needs no table, and a
//    batch has up to 65535 problems).  It travels by value and is read with one uniform load of the word that holds the byte.
//  - the table has two dimensions where the launch has a controller axis in blockIdx.z (jh_plan_step_randomized_batch: every controller draws its own assignment):
//    the entry of (controller c, problem b) is c * gridDim.y + b, controller-major, JH_MAX_FLEET_PLANT_BLOCKS entries in all.  With gridDim.z == 1 that is b.
// Both are wave-uniform arithmetic on kernel arguments and the block indices, done once at the top of the kernel.
struct jh_plant_axis {
  int n_stride = 0;
  unsigned mapped = 0;
  unsigned plant[JH_MAX_FLEET_PLANT_BLOCKS / 4] = {};
};
// the image of problem b, whose entry of the table is e (e == b in a launch without a controller axis)
__host__ __device__ inline int jh_plant_of(const jh_plant_axis& p, int e, int b) { return p.mapped ? (int)((p.plant[e >> 2] >> ((e & 3) << 3)) & 0xffu) : b; }
inline void jh_plant_set(jh_plant_axis& p, int e, int plant) { p.mapped = 1u; p.plant[e >> 2] |= (unsigned)(plant & 0xff) << ((e & 3) << 3); }

// What the leap kernel's launch for B problems (jh_plan_step_batch) takes on top: the record is problem 0's, `blk_stride` / `noise_stride` floats lead to the next problem's;
// `images`: problem 0's float section, `image_stride` floats to the next problem's (m->d_f and 0: one image for all); `ints`: the int section on the device (m->d_i, or a
// model set's copy without the hand's pair tables).  `C` > 1 (jh_plan_step_ensemble_batch): the launch has a controller axis in front of the problems -- the grid is
// (groups, B, C), controller c's blocks, noise and images lie c times the `*_stride_c` floats behind controller 0's, and the (controller, problem) pair c * B + b owns the
// costs, trace and overflow rows.  The default is the launch without that axis.
// `plants` (jh_plan_step_randomized): the problems are slices of ONE problem's rollouts, each on a plant of the set -- problem b's global rollout index starts
// plants.n_stride behind problem b - 1's, and its image is plants' table entry b instead of b (entry c * B + b with a controller axis, jh_plan_step_randomized_batch).  The default, 0 and the identity, is every
// other launch.
// `o_phase` (jh_plan_step_batch_phases, the fr3 kernel alone): the float offset of the problem's phase word in its packed block, whose first word is the record's x0 --
// the one argument of the single launch that is a problem's own.  -1: the launch has no phase word (the leap kernel ignores the field), and the fr3 kernel takes
// `phase`, 0..3, for every problem: the problems are blocks of one controller's rollouts (jh_plan_step_randomized_phase), and one controller has one phase.  `phase` is
// read only when o_phase < 0.  The fr3 launcher implements the images and the plant axis as the leap launcher does, reads the model's own int section (fr3_pick has no
// pair tables; `ints` is not used), and the controller axis as well: C up to 65535, C * B * N rollouts in one launch.
struct jh_rollout_batch {
  const float* images; long long image_stride; const int* ints;
  int B; long long blk_stride, noise_stride;
  int C = 1; long long blk_stride_c = 0, noise_stride_c = 0, image_stride_c = 0;
  jh_plant_axis plants = {};
  int o_phase = -1;
  int phase = -1;
};

// The trace sensors a fused kernel writes per rollout and step: the first sensor address, the number of floats (0: none -- the elites are re-rolled in materialise mode
// instead) and whether the buffer is column-major (one lane per rollout) or a row per rollout.
struct jh_trace_layout { int adr = 0, floats = 0, colmajor = 0; };
namespace jh_upd { struct TailArgs; struct BatchArgs; }  // (jh_update_dev.h: the update tail's kernel arguments, which the one-launch plan step takes as they are)

// One build of a product kernel: each translation unit that instantiates k_leap_v5 or k_fr3_v6 defines its row, jh_simple.hip one for the two closed-form models, and
// jh_api.hip's engine_build() maps a model to the row that runs it.  A new build is a new row and a line of that function.
struct jh_engine_build {
  const char* name;                       // for messages
  bool (*accepts)(const jh_model* m);     // the launchers' own acceptance test, on the model's own image
  int (*rollout_cost)(const jh_model* m, const jh_rollout_args& a, hipStream_t st);
  int (*rollout_cost_batch)(const jh_model* m, const jh_rollout_args& a, const jh_rollout_batch& s, hipStream_t st);  // null: the build has no batched launch (none of the shipped rows; fr3: a phase per problem, jh_rollout_batch::o_phase)
  int (*materialize)(const jh_model* m, const float* x0, int x0_batched, const float* controls, int N, int H, float* states, float* sensors, hipStream_t st);
  int contact_capacity;                   // contacts a rollout can hold (jh_model_limits out[3]), from the build's own constants
  // materialise mode on a plant axis (jh_rollout_materialize_plants; the fr3 rows: jh_fr3_rollout_materialize_plants): s.B blocks of n rollouts, block g on image
  // s.plants[g] of s.images; of `s` the launch reads images, image_stride, ints, B and plants -- the fr3 rows the model's own int section in place of `ints`, and C, which
  // they refuse unless it is 1.  null: the build has no such launch (none of the shipped rows)
  int (*materialize_plants)(const jh_model* m, const jh_rollout_batch& s, const float* x0, int x0_batched, const float* controls, int controls_shared, int n, int H, float* states,
                            float* sensors, hipStream_t st) = nullptr;
  int (*max_fused_knots)(const jh_model* m, int H) = nullptr;    // the build's own bound on a fused launch's K at horizon H, under JH_MAX_KNOT_DIM / nu (jh_model_max_fused_knots); null: none of its own
  jh_trace_layout (*trace_layout)(const jh_model* m) = nullptr;  // what a fused launch with a trace buffer writes (jh_model_trace_layout); null: this build writes no trace
  // The plan step as ONE launch, rollout + cost + the update's tail (jh_model_set_plan_step_launches): the largest K whose staging fits at horizon H, the launch on the
  // tail's own record, and the batched launch on problem 0's record, `images` as in jh_rollout_batch and s.image floats apart.  All null: a build whose plan step is two
  // launches (every articulated row).
  int (*one_launch_max_knots)(const jh_model* m, int H) = nullptr;
  int (*plan_step)(const jh_model* m, const float* x0, const float* W, const float* tp, int H, int K, const jh_upd::TailArgs& a, hipStream_t st) = nullptr;
  int (*plan_step_batch)(const jh_model* m, const float* images, const float* x0, const float* W, const float* tp, int H, int K, const jh_upd::TailArgs& a, const jh_upd::BatchArgs& s,
                         hipStream_t st) = nullptr;
};
// (hidden: the rows are the library's own, not part of its boundary)
extern __attribute__((visibility("hidden"))) const jh_engine_build jh_simple_build;  // jh_simple.hip: cartpole and cylinder_push, one row for both (contact capacity 0: neither model holds contacts in a pool)
extern __attribute__((visibility("hidden"))) const jh_engine_build jh_engine5_build, jh_engine5_build_cap64, jh_engine5_build_cyl;  // jh_engine_v5.hip: the leap kernel for 48 and 64 contacts, and with cylinders
extern __attribute__((visibility("hidden"))) const jh_engine_build jh_engine6_build, jh_engine6_build_self;  // jh_engine_v6.hip: the fr3 kernel, and with the arm's own pairs (jh_model::arm_pairs > 0)

// jh_api.hip: what jh_plants.hip reads of a model set (the structure is that file's own): member 0, whose kind and dimensions are the set's, and the members
__attribute__((visibility("hidden"))) const jh_model* jh_model_set_member0(const jh_model_set* set);
__attribute__((visibility("hidden"))) int jh_model_set_members(const jh_model_set* set);

// The words of jh_model::d_stats that every product build writes and the host reads (jh_model_stats, jh_model_recomputed_units): contact-cap overflows, Newton iteration-cap
// hits, Newton iterations, steps; wave-level iterations, steps; leap queue units whose hand-off was missed and which recomputed their group up to their slice.  The rest
// belongs to diagnostic builds.
enum { JH_STAT_DROPS = 0, JH_STAT_ITER_CAP, JH_STAT_ITERS, JH_STAT_STEPS, JH_STAT_WAVE_ITERS = 20, JH_STAT_WAVE_STEPS, JH_STAT_RECOMPUTED = 56 };

// Latency mode of the cooperative kernels (rows of `lanes` lanes, `rpw` rows per wave): a launch too small to give every SIMD a wave lets 1 << shift rows of a wave
// compute the same rollout -- the copies run the same arithmetic, only the first writes -- so that a wave no longer waits for the slowest of `rpw` different Newton
// solves in every step.  Returns the largest shift (<= log2 rpw) that still leaves every wave of the launch a SIMD of its own; JUDO_AMD_LATENCY_SHIFT=0..2 overrides.
int jh_latency_shift(int N, int rpw);
int jh_engine_max_knots(const jh_model* m, int H);
int jh_simple_reward(const jh_model* m, const float* states, const float* controls, const float* tp, int N, int H, float* rewards, hipStream_t st);  // (jh_task_reward: the one closed-form launcher outside the row)

int jh_engine_rollout_cost(const jh_model* m, const float* x0, const float* nominal, const float* noise, int ldn, const float* sigma,
                           const float* W, const float* lohi, const float* tp, int phase, int N, int n_offset, int H, int K, float* costs,
                           float* knots_out, hipStream_t st);
int jh_engine_materialize(const jh_model* m, const float* x0, int x0_batched, const float* controls, int N, int H, float* states,
                          float* sensors, hipStream_t st);
int jh_engine_reward(const jh_model* m, const float* states, const float* sensors, const float* controls, const float* tp, int phase, int N,
                     int H, float* rewards, hipStream_t st);

int jh_engine2_rollout_cost(const jh_model* m, const float* x0, const float* nominal, const float* noise, int ldn, const float* sigma,
                            const float* W, const float* lohi, const float* tp, int N, int n_offset, int H, int K, float* costs, float* knots_out,
                            hipStream_t st);
int jh_engine2_materialize(const jh_model* m, const float* x0, int x0_batched, const float* controls, int N, int H, float* states, float* sensors,
                           hipStream_t st);

// jh_engine_v3.hip: cooperative kernel for fr3_pick (serial arm with a two-finger fork + free box, pyramidal cones)
bool jh_model_is_fr3(const jh_model* m);  // (defined by jh_engine_v6.hip: the default build's acceptance test, which the cross-check kernel shares)
int jh_engine3_rollout_cost(const jh_model* m, const float* x0, const float* nominal, const float* noise, int ldn, const float* sigma, const float* W,
                            const float* lohi, const float* tp, int phase, int N, int n_offset, int H, int K, float* costs, float* knots_out, hipStream_t st);
int jh_engine3_materialize(const jh_model* m, const float* x0, int x0_batched, const float* controls, int N, int H, float* states, float* sensors,
                           hipStream_t st);

// ---- device helpers ------------------------------------------------------------------------------------------
// MuJoCo's impedance curve d(x) (solimp = dmin, dmax, width, midpoint, power), x = |pos - margin| / width.
__device__ __forceinline__ float jh_impedance(float s0, float s1, float s2, float s3, float s4, float dist) {
  if (s0 == s1 || s2 <= 1e-15f) return 0.5f * (s0 + s1);
  float x = fabsf(dist / s2);
  if (x >= 1.f) return s1;
  if (x <= 0.f) return s0;
  float y;
  if (s4 == 1.f) y = x;
  else if (x <= s3) y = __powf(x, s4) / __powf(s3, s4 - 1.f);
  else y = 1.f - __powf(1.f - x, s4) / __powf(1.f - s3, s4 - 1.f);
  return s0 + y * (s1 - s0);
}

__device__ __forceinline__ float jh_clampf(float v, float lo, float hi) { return fminf(hi, fmaxf(lo, v)); }

// jh_policy.hip: one policy step with explicit row strides (used by the policy rollout loop in jh_engine_v4.hip)
struct jh_policy;
int jh_policy_step_strided(const jh_policy* p, const float* states, int ld, int nq, int base_qpos, int base_qvel, int leg_qpos, int leg_qvel, const float* command, int ldc,
                           float* policy_out, float* control, float* scratch, int N, hipStream_t st);
