/*
 * judo_amd.h -- C ABI of libjudo_amd.so: the MI355X (gfx950) sampling-MPC rollout engine.
 *
 * Drop-in boundary for the hot path of bdaiinstitute/judo v0.0.7
 * (sample -> clip -> spline -> rollout -> cost -> update).  The reference has no C ABI of its own for
 * this path: the seam is three Python ABCs (Optimizer, RolloutBackend, Task) plus the pybind11 module
 * mujoco_extensions/policy_rollout.  Each entry point below names the reference interface it replaces;
 * INTEGRATION.md shows the ctypes binding a judo maintainer would add.
 *
 * Conventions
 *   - every `const float*` / `float*` is a DEVICE pointer (fp32, contiguous) unless marked HOST;
 *   - `stream` is a hipStream_t passed as void* (0 = the null stream); all work is enqueued
 *     asynchronously on it, nothing synchronises;
 *   - the caller owns every buffer; the library owns only jh_model handles (model constants in device
 *     memory) -- no hidden allocation on the step path;
 *   - return 0 on success, a negative jh_status otherwise; jh_last_error() gives the message
 *     (thread-local).  Functions are re-entrant per jh_model.
 *   - rollouts are indexed n = 0..N-1 locally, n_offset + n globally; global sample 0 is the
 *     unperturbed nominal (judo/optimizers/mppi.py:59 `concatenate([nominal[None], noised])`).
 *   - noise layout is (K, nu, ldn) with the rollout index fastest (64 consecutive lanes read 256
 *     contiguous bytes); element (k,u,n) at noise[(k*nu+u)*ldn + n].
 */
#ifndef JUDO_AMD_H
#define JUDO_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct jh_model jh_model;

enum jh_status {
  JH_OK = 0,
  JH_ERR_INVALID = -1,   /* bad argument (shape, null pointer, unsupported size) */
  JH_ERR_HIP = -2,       /* HIP runtime error */
  JH_ERR_UNSUPPORTED = -3,
  JH_ERR_BLOB = -4       /* malformed model blob */
};

enum jh_task_kind { JH_TASK_CARTPOLE = 0, JH_TASK_CYLINDER_PUSH = 1, JH_TASK_LEAP_CUBE = 2, JH_TASK_FR3_PICK = 3 };
enum jh_spline_kind { JH_SPLINE_ZERO = 0, JH_SPLINE_LINEAR = 1, JH_SPLINE_CUBIC = 3 };

#define JH_MAX_TASK_PARAMS 32
#define JH_MAX_KNOT_DIM 512 /* K * nu */
#define JH_MAX_ELITES 32
#define JH_MAX_ENSEMBLE 32 /* members of a model set that jh_plan_step_ensemble plans against */
#define JH_MAX_ENSEMBLE_FLEET 256 /* controllers of one jh_plan_step_ensemble_batch call (their `worst` travel in the kernel arguments, a byte each) */
#define JH_MAX_PLANT_BLOCKS 64 /* rollout blocks of one jh_plan_step_randomized call (their plants travel in the kernel arguments, a byte each) */
#define JH_MAX_FLEET_PLANT_BLOCKS 256 /* B * G, the (controller, block) pairs of one jh_plan_step_randomized_batch call: the bytes of its table in the kernel arguments */
#define JH_MAX_ID_HORIZON 64 /* steps of a recorded window that jh_plant_residuals scores: the wave width, a lane per step */
#define JH_MAX_ID_QUATS 4 /* quaternions of a state row that jh_plant_residuals aligns (their offsets travel in the kernel arguments) */

const char* jh_last_error(void);
int jh_version(void);

/* Model constants (the MjModel the reference deep-copies per thread, judo/utils/mj_rollout_backend.py:41):
 * `blob` is a HOST buffer produced by judo_amd.models.pack_model(); it is parsed and uploaded to `device`. */
int jh_model_create(const void* blob, size_t nbytes, int device, jh_model** out);
void jh_model_destroy(jh_model* m);
/* dims[0..5] = nq, nv, nu, nsensordata, task kind, ntaskparams */
int jh_model_dims(const jh_model* m, int* dims /* HOST */);

/* Diagnostics accumulated by the articulated-body kernels since the last reset (synchronises the device):
 * out[0] contacts dropped because a rollout exceeded the per-rollout contact capacity, out[1] constraint solves that hit the
 * Newton iteration cap, out[2] Newton iterations (summed over rollouts), out[3] physics steps (summed over rollouts); leap_cube kernel generation 3 also:
 * out[4] Newton iterations executed by wavefronts (four rollouts advance in lock step: per step the maximum over the four), out[5] physics steps
 * summed over wavefronts; out[6] launches that ran without their overflow rows because the device's memory pool refused the scratch block (the contact capacity was then what
 * the LDS pool holds); out[7] plan steps of jh_plan_step / jh_plan_step_shard that ran as one launch (cartpole, cylinder_push; counted on the host, no device work).  The counters are 32-bit and wrap: reset them at least every ~10^9 rollout-steps.  HOST pointer. */
int jh_model_stats(jh_model* m, int* out /* HOST, 8 ints */, int reset);

/* (The cross-check kernel generations of the parity tests and their registration hook are NOT part of this interface: include/judo_amd_xcheck.h.) */

/* leap_cube on kernel generation 3: model the hand's own contacts (every finger-finger / finger-palm geom pair MuJoCo's filters leave: same welded body,
 * parent-child, the 18 <exclude> pairs of leap_components/params_and_default.xml:76-101) next to the cube's -- the default, MuJoCo collides them -- or,
 * with on = 0, the cube's contacts alone (what generations 1 and 2 model). */
int jh_model_set_self_collision(jh_model* m, int on);

/* leap_cube family, kernel generation 3: contacts a rollout can hold.  48 (default: all in LDS) or 64 (a second build of the kernel, jh_engine_v5_cap64.hip: the 16 above the LDS
 * pool in a per-rollout row of global memory; 2.8 % slower on every plan step).  The headline workload drops 2e-6 contacts per rollout-step at 48; the shipped leap_cube_down and
 * caltech_leap_cube workloads 2e-4 .. 4e-4, which is why judo_amd selects 64 for those two models.  jh_model_limits out[3] reports the setting. */
int jh_model_set_contact_capacity(jh_model* m, int contacts);

/* Which build of its kernel a model runs: out[0] = kernel generation, out[1] = contact capacity of the leap kernel's build (48 or 64; 0: another kernel), out[2] = 1 when
 * that is the CYLINDER build (jh_engine_v5_cyl.hip), out[3] = cylinder geoms in the image.  The cylinder build is selected by the image, not by a setter: an image of the
 * leap family that keeps caltech_leap_cube's fingertip cylinders (geom type 5, sizes (radius, half length), bounding radius sqrt(r^2 + L^2); engine_model.py,
 * fingertips="cylinder") runs sphere-cylinder through MuJoCo's primitive and box-cylinder / cylinder-cylinder through a bounded fp32 GJK + EPA, at 64 contacts per
 * rollout.  jh_model_create refuses a malformed cylinder record and a cylinder in any other family; kernel generations 1 and 2 and the 48-contact setting refuse such a
 * model; the sphere builds refuse its image.  HOST pointer. */
int jh_model_build(const jh_model* m, int* out /* HOST, 4 ints */);

/* The same report for the fr3_pick kernel: out[0] = 1 when the model runs the SELF-COLLISION build (jh_engine_v6_self.hip), out[1] = the image's candidate pairs the
 * default build leaves out (between two arm bodies other than finger against finger, or a box on the arm against the capsule of the static base), out[2] / out[3] = 1
 * when the default / the self-collision build accepts the image.  Selected by the image, as the cylinder build is: an image packed from a description with
 * "self_collision" (engine_model.py; FR3Pick(self_collision=True)) holds all 190 pairs the MJCF leaves after MuJoCo's static filters, the default image 78.  The
 * self-collision build takes capsule against capsule (MuJoCo's primitive) and a contact with both sides on the arm.  jh_model_create refuses a malformed pair of that
 * kind; kernel generations 1 and 2 refuse such a model; the default build refuses its image.  Another model family: all zero.  HOST pointer. */
int jh_model_fr3_build(const jh_model* m, int* out /* HOST, 4 ints */);

/* Traces without a second rollout (judo/controller/controller.py:323-363, `update_traces`: line segments of the best rollouts' `trace*` framepos sensors).  The
 * reference reads them out of the sensor array its rollout materialises for every sample; the fused path has no such array, so round 1-2 re-rolled the elites in
 * materialise mode when the traces were read (8 ms on the headline workload: one lone wave for 64 serial steps).  jh_rollout_cost_traced (jh_rollout_cost with one more argument) on
 * leap_cube / fr3_pick (kernel generation 3), cartpole and cylinder_push also writes the trace sensors of EVERY rollout and step into `trace`: row n (rollout index within the launch) holds
 * H x out[1] floats, the sensors out[0] .. out[0] + out[1] - 1 of jh_model_trace_layout (leap_cube: 16, 15 = five site positions; fr3_pick: 8, 6; cartpole,
 * cylinder_push: 0, 6; out[1] = 0: the model's kernel writes none).  out[2] = 1: the buffer is column-major -- element i of rollout n at [i * N + n] (the one-lane-
 * per-rollout kernels of cartpole / cylinder_push: coalesced) -- else row-major, [n * H * out[1] + i].  60 B per rollout-step, a few hundred MB per plan step that
 * nobody reads back except the elites' rows: jh_trace_gather copies, for each record [cost, global index (bits), ...] of a jh_topk_partial result, the row of that
 * rollout behind cost and index -- the payload the ranks exchange. */
int jh_model_trace_layout(const jh_model* m, int* out /* HOST, 3 ints */);
int jh_trace_gather(const float* rec_in /* DEVICE, k x stride_in */, int k, int stride_in, int n_offset, int n_local, const float* trace /* DEVICE */, int row_floats,
                    int colmajor, float* rec_out /* DEVICE, k x (2 + row_floats) */, void* stream);

/* Small launches (latency mode): when N rollouts would leave SIMDs idle, the cooperative kernels (leap_cube, fr3_pick: four rows of 16 lanes per wave; Spot tree: two
 * rows of 32) let 4 or 2 rows of a wave compute the same rollout -- identical arithmetic, the first row writes -- so that a wave does not wait for the slowest of
 * its different rollouts' Newton solves in every step.  Results are bit-identical to the full mapping.  Chosen per launch from N and the CU count; the environment
 * variable JUDO_AMD_LATENCY_SHIFT=0 switches it off (1 / 2: force two / four copies). */
/* Limits of this model's kernels: out[0] = largest knot count K the fused kernel (jh_rollout_cost) accepts -- the cooperative fr3_pick kernel
 * keeps a lane's knots on chip (8 of them); the leap_cube kernel of generation 3 reads them from memory every step and is bounded by
 * JH_MAX_KNOT_DIM / nu alone.  A larger K goes through jh_spline_controls + jh_rollout_materialize + jh_task_reward, which have no such limit;
 * out[1] = JH_MAX_KNOT_DIM; out[2] = JH_MAX_ELITES; out[3] = contact capacity per rollout of the general pool (leap_cube generation 3: 48 or 64, jh_model_set_contact_capacity;
 * fr3_pick generation 3: 96 -- 32 on chip, 64 in a row of global memory -- next to its 96 pad-against-pad slots; 0 = the model has at most one contact).  HOST pointer. */
int jh_model_limits(const jh_model* m, int* out /* HOST, 4 ints */);
/* out[0] of jh_model_limits is an upper bound over all horizons.  The one-lane kernels (cartpole, cylinder_push, kernel generation 1) stage W (H x K) and
 * their lanes' knots in LDS, so their largest fused K also depends on the horizon: this returns the K up to which jh_rollout_cost accepts a launch of H
 * steps (>= 0), or a negative jh_status.  A Controller asks before every plan step and takes the materialise path above it (a live num_nodes / horizon
 * edit, judo/optimizers/base.py:15-21, must not raise out of update_action). */
int jh_model_max_fused_knots(const jh_model* m, int H);
/* The closed-form models (cartpole, cylinder_push) run a plan step of jh_plan_step as ONE launch (rollout + cost + update tail) when the knots of a workgroup of 256
 * rollouts and W fit its 48 KiB LDS staging: this returns the largest such K at horizon H (<= jh_model_max_fused_knots; 0 for the other models), or a negative jh_status.
 * Above it the plan step takes two launches, the fused rollout kernel and then the update tail; both forms give the same bits. */
int jh_model_one_launch_max_knots(const jh_model* m, int H);
/* How jh_plan_step / jh_plan_step_shard run a closed-form model's plan step: 0 = one launch up to jh_model_one_launch_max_knots, two above (the default), 1 = always one
 * launch (a plan step it cannot hold -- K above the limit, or knots_out requested -- fails with JH_ERR_INVALID), 2 = always two.  The environment variable
 * JUDO_AMD_PLAN_STEP_LAUNCHES=2 makes 2 the default of every model created after it is set.  1 is refused for the articulated models, which always take two. */
int jh_model_set_plan_step_launches(jh_model* m, int launches);
/* How the fused leap_cube kernel of generation 3 (jh_rollout_cost, jh_plan_step ...) places its groups of four rollouts on the GPU: 0 = automatic (the default): a launch with
 * more groups than the GPU holds waves of the kernel at once starts one workgroup per resident slot, and every wave draws group after group from a per-launch queue
 * (persistent waves); a launch that fits at once, and every latency-mode launch, has one group per wave of its grid.  1 = always the static grid.  2 = the queue wherever
 * the kernel has it (every fused launch outside the latency mode).  All three give the same bits: a rollout's result does not depend on the wave that runs it.  The
 * environment variable JUDO_AMD_ROLLOUT_SCHEDULE=1 / 2 sets the default of every model created after it is set.  Accepted and without effect on the other models. */
int jh_model_set_rollout_schedule(jh_model* m, int mode);
/* The units of that queue.  `slices`: 0 = automatic (the default): a launch that runs the queue AND has at least two groups per resident wave splits every group's horizon
 * into slices, and a queue unit is (group, slice) -- all first slices, then all second ones -- so that the launch drains over a slice's duration instead of a group's; every
 * other launch keeps whole groups.  1 .. 64 forces that many slices (clipped to the horizon) wherever the queue runs; 1 = whole groups.  A slice hands the rollouts' state
 * to the next one through the launch's scratch and a flag that is read once, never waited for: a wave that finds it unset recomputes the group's steps up to its slice.
 * `max_workgroups`: 0 = one workgroup per resident slot; > 0 caps the queue's grid (a test hook: a small launch then draws tickets and hands states over).  `flags` bit 0:
 * every hand-off counts as missed (a test hook for the recomputation).  None of this changes a bit of any output.  Other values: JH_ERR_INVALID.  Accepted and without
 * effect on the other models.  The environment variable JUDO_AMD_ROLLOUT_SLICES=1 .. 64 sets the default `slices` of every model created after it is set. */
int jh_model_set_rollout_slices(jh_model* m, int slices, int max_workgroups, int flags);
/* An explicit schedule of that queue's slices, which need not be equal: `first_steps[0 .. n)` are the first steps of slices 1 .. n (slice 0 starts at step 0), positive and
 * strictly increasing, n <= 15 (at most 16 slices); n = 0 clears it.  At a launch, entries at or behind the horizon are dropped, so one schedule serves any horizon; what is
 * left runs wherever the queue runs.  Of this setter and jh_model_set_rollout_slices THE LATER CALL DECIDES the slices: setting a schedule (n > 0) puts `slices` back to 0 and
 * leaves `max_workgroups` and `flags` as they are, and every call of jh_model_set_rollout_slices clears the schedule.  With neither, the automatic rule below.  None of this
 * changes a bit of any output.  Other values: JH_ERR_INVALID.  The environment variable JUDO_AMD_ROLLOUT_SLICE_BOUNDS=a,b,... sets the default of every model created after
 * it is set (and goes in front of JUDO_AMD_ROLLOUT_SLICES). */
int jh_model_set_rollout_slice_bounds(jh_model* m, const int* first_steps, int n);
/* What the model's last fused leap_cube launch of generation 3 ran: 0 = the static grid, 1 = the queue of whole groups, S > 1 = the queue of S slices per group. */
int jh_model_last_rollout_slices(const jh_model* m);
/* The first steps of slices 1 .. S - 1 of that launch (equal slices: s H / S): at most `cap` of them go to `out`, the return value is their number (0 for whole groups and for
 * the static grid), or a negative jh_status. */
int jh_model_last_rollout_slice_bounds(const jh_model* m, int* out, int cap);
/* The automatic schedule as a pure function (no model, no device): a fused launch of `groups` groups of four rollouts over `H` steps on a GPU that holds `wave_slots` waves of
 * the kernel (8 per CU).  Fewer than two groups per slot: whole groups (returns 0).  From two: four equal slices (H = 8: 2, 4, 6).  From four groups per slot and H >= 32:
 * five slices of 3/8, 1/4, 3/16, 1/8 and 1/16 of the horizon (H = 64: 24, 40, 52, 60), so that the units drawn last, over which the launch drains, are short.  At most `cap`
 * first steps go to `first_steps`; the return value is their number, or a negative jh_status.  Every first step is inside (0, H). */
int jh_rollout_slice_schedule(int H, int groups, int wave_slots, int* first_steps, int cap);
/* Queue units that found their hand-off unset and recomputed their group up to their slice, summed over the model's launches since the counters were last reset
 * (jh_model_stats with reset != 0); synchronises.  A negative jh_status on failure. */
int jh_model_recomputed_units(jh_model* m);

/* Plan-step I/O in one call each (the two transfers of a plan step: < 2 KB down, the new nominal knots up): an asynchronous copy of `nbytes` from
 * pinned HOST memory to the device on `stream`; and an asynchronous copy from the device to pinned HOST memory followed by a wait for `stream`
 * (the only synchronisation of an optimiser iteration, judo/controller/controller.py:283 needs the new nominal on the host). */
int jh_upload_async(void* dst_device, const void* src_host, size_t nbytes, void* stream);
int jh_download_wait(void* dst_host, const void* src_device, size_t nbytes, void* stream);
/* The same in two halves: `begin` enqueues the copy and marks its end on `stream`; work enqueued afterwards (the trace records of update_traces)
 * runs behind it; `end` waits for the mark only.  Marks are kept per host thread and stream (a thread may drive controllers on several GPUs) and `end`
 * waits for the oldest mark of the calling thread that has not been waited for yet; a stream carries one mark at a time. */
int jh_download_begin(void* dst_host, const void* src_device, size_t nbytes, void* stream);
int jh_download_end(void);

/* Fused plan-step kernel.  Replaces, for N rollouts in one launch:
 *   Optimizer.sample_control_knots         judo/optimizers/{mppi.py:38-59,ps.py:29-50,cem.py:55-74}
 *   np.clip to actuator_ctrlrange          judo/controller/controller.py:253-257
 *   make_spline(...)(t + dt*arange(H))     judo/controller/controller.py:261-262  (as the H x K matrix W)
 *   RolloutBackend.rollout                 judo/utils/mj_rollout_backend.py:45-88 (mj_step x H)
 *   Task.reward                            judo/tasks/{cartpole.py:42,cylinder_push.py:50,leap_cube.py:63,fr3_pick.py:225}
 * costs[n] = -reward of rollout n.  knots_out (optional, may be NULL) receives the clipped candidates in
 * (K, nu, ldn) layout.  `phase` is the fr3_pick phase chosen on the host by Task.pre_rollout
 * (judo/tasks/fr3_pick.py:191-223); ignored by the other tasks. */
int jh_rollout_cost(const jh_model* m, const float* x0, const float* nominal, const float* noise, int ldn, const float* sigma,
                    const float* W, const float* ctrl_lo_hi, const float* task_params, int phase, int N, int n_offset, int H, int K,
                    float* costs, float* knots_out, void* stream);
int jh_rollout_cost_traced(const jh_model* m, const float* x0, const float* nominal, const float* noise, int ldn, const float* sigma,
                    const float* W, const float* ctrl_lo_hi, const float* task_params, int phase, int N, int n_offset, int H, int K,
                    float* costs, float* knots_out, float* trace /* DEVICE, N x H x jh_model_trace_layout out[1] floats, or NULL */, void* stream);

/* Drop-in RolloutBackend.rollout(x0, controls) -> (states, sensors)   judo/utils/rollout_backend.py:20-39.
 * controls (N,H,nu), states (N,H,nq+nv), sensors (N,H,nsensordata), all row-major; x0 is (nq+nv) or, when
 * x0_batched, (N,nq+nv).  states[n,h] is the state AFTER applying controls[n,h]; sensors[n,h] is what the
 * forward pass at the start of that step computed (MuJoCo semantics). */
int jh_rollout_materialize(const jh_model* m, const float* x0, int x0_batched, const float* controls, int N, int H, float* states,
                           float* sensors, void* stream);

/* Task.reward on materialised device arrays (same task_params as jh_rollout_cost); rewards[n] (not negated). */
int jh_task_reward(const jh_model* m, const float* states, const float* sensors, const float* controls, const float* task_params,
                   int phase, int N, int H, float* rewards, void* stream);

/* The optimizers' noise, `np.random.randn(num_rollouts - 1, num_nodes, nu)` of judo/optimizers/{mppi.py:52,ps.py:43,cem.py:67}, drawn on the device in the
 * kernels' layout: out[row * ldn + n] for row < rows (= K * nu) and local rollout n < n_local is the standard normal that belongs to GLOBAL rollout
 * n_offset + n of draw number `draw` under `seed` (Philox4x32-10, counter-based: a pure function of seed, draw, row and the global rollout index, two
 * Box-Muller pairs per block of four rollouts).  A rank generates exactly its shard's columns; the plan does not depend on the number of GPUs. */
int jh_noise_normal(unsigned long long seed, unsigned int draw, int rows, int n_offset, int n_local, float* out, int ldn, void* stream);

/* Optimizer.sample_control_knots for callers that want the (N,K,nu) row-major array itself
 * (row n = nominal + sigma * noise[:, :, n], row 0 of global index 0 = nominal), optionally clipped. */
int jh_sample_knots(const float* nominal, const float* noise, int ldn, const float* sigma, const float* ctrl_lo_hi /* NULL = no clip */,
                    int N, int n_offset, int K, int nu, float* knots_nku, void* stream);

/* Candidate control trajectories of the materialise path (judo/controller/controller.py:239-249: the candidate splines evaluated at
 * the rollout times): controls[n,h,u] = sum_k W[h,k] * knot(n,k,u), (N,H,nu) row-major, ready for jh_rollout_materialize.
 * W is the (H,K) interpolation matrix of the spline kind (linear in the knots for zero/linear/cubic interp1d); knots come from
 * `knots_nku` or, when it is NULL, are recomputed as clip(nominal + sigma*noise) exactly like jh_rollout_cost does.  Every K * nu <= JH_MAX_KNOT_DIM and every H:
 * W and the knots are staged in LDS where they fit and read from global memory where they do not (same bits). */
int jh_spline_controls(const float* W, const float* knots_nku, const float* nominal, const float* noise, int ldn, const float* sigma,
                       const float* ctrl_lo_hi, int N, int n_offset, int H, int K, int nu, float* controls, void* stream);

/* Moments of this shard's candidate knots for the "running" action normaliser (RunningMeanStdNormalizer.update on candidate_knots,
 * judo/utils/normalization.py:176-200, judo/controller/controller.py:290-291): out[u] = sum over rollouts and knots of (x - center[u]),
 * out[nu+u] = sum of (x - center[u])^2, x = knot of actuator u (same knot sources as jh_spline_controls).  `out` (2*nu floats) is zeroed first. */
int jh_knot_moments(const float* knots_nku, const float* nominal, const float* noise, int ldn, const float* sigma, const float* ctrl_lo_hi,
                    const float* center, int N, int n_offset, int K, int nu, float* out, void* stream);

/* MPPI.update_nominal_knots (judo/optimizers/mppi.py:61-82), shard-local part.
 * Writes one record rec[0] = beta = min cost, rec[1] = S = sum exp(-(c-beta)/lambda), rec[2..2+K*nu) = sum w*knots.
 * Knots come either from `knots_nku` ((N,K,nu) row-major, the drop-in path) or, when it is NULL, are recomputed as
 * clip(nominal + sigma*noise) from the (K,nu,ldn) noise (the fused path: noise is read once more, never stored).
 * `scratch` must hold jh_update_scratch_floats(N,K,nu) floats. */
size_t jh_update_scratch_floats(int N, int K, int nu);
int jh_mppi_partial(const float* costs, const float* knots_nku, const float* nominal, const float* noise, int ldn, const float* sigma,
                    const float* ctrl_lo_hi, int N, int n_offset, int K, int nu, float lambda, float* scratch, float* rec, void* stream);
/* Merge G shard records (after the all-gather) with a log-sum-exp rescale: nominal_out = sum_g e_g V_g / sum_g e_g S_g,
 * e_g = exp(-(beta_g - min beta)/lambda).  Identical result on every rank. */
int jh_mppi_merge(const float* recs, int G, int K, int nu, float lambda, float* nominal_out, void* stream);

/* CrossEntropyMethod / PredictiveSampling updates (judo/optimizers/cem.py:76-92, ps.py:52-65), shard-local part:
 * the k best rollouts (largest reward = smallest cost; ties: higher global index first when tie_high != 0, which is
 * what flip(argsort(.)) yields for a stable sort, lower index first otherwise = np.argmax), each as a record
 * [cost, global index, knots(K*nu)].  rec holds k such records. */
int jh_topk_partial(const float* costs, const float* knots_nku, const float* nominal, const float* noise, int ldn, const float* sigma,
                    const float* ctrl_lo_hi, int N, int n_offset, int K, int nu, int k, int tie_high, float* scratch, float* rec,
                    void* stream);
/* The whole update of a ONE-GPU plan step in one launch (Controller.update_action's tail, judo/controller/controller.py:288-299): what jh_mppi_partial + jh_mppi_merge
 * (mode 0) or jh_topk_partial + jh_elite_merge (mode 1: k elites, raw population std into sigma_out, which may be NULL) compute, plus -- when E > 0 -- the records
 * [cost, global index (bits), trace row] of the E best rollouts (ties: higher index first) that jh_topk_partial + jh_trace_gather produce, into trace_out (E x (2 + row_floats)).
 * Every workgroup writes its partial records to `scratch` and the last one to finish merges them: same arithmetic in the same order as the separate calls, bit-identical
 * outputs.  `scratch`: jh_update_fused_scratch_floats(N, K, nu) floats, ZERO before its first use (it holds the ticket counter, which every launch leaves at zero).
 * NaN costs (a diverged rollout) deviate from the reference on purpose: the update takes a NaN cost for +inf -- MPPI weight zero, ranked behind every finite cost
 * for the CEM / PS elites and the trace elites -- where numpy would let it poison the weighted mean, win np.argmax and sort first in flip(argsort).  A trace record whose
 * rollout's cost is +inf or NaN (>= 3e38), or that lies past the last rollout (E > N), is empty: cost +inf, index -1, zero row.  With no finite cost at all the MPPI
 * mean is NaN, as the reference's is. */
size_t jh_update_fused_scratch_floats(int N, int K, int nu);
int jh_update_fused(const float* costs, const float* knots_nku, const float* nominal, const float* noise, int ldn, const float* sigma, const float* ctrl_lo_hi, int N,
                    int n_offset, int K, int nu, int mode, float lambda, int k, int tie_high, int E, const float* trace, int row_floats, int colmajor, float* scratch,
                    float* nominal_out, float* sigma_out, float* trace_out, void* stream);
/* One iteration of Controller.update_action's loop (judo/controller/controller.py:250-299) on ONE GPU as one call: upload of the packed host block
 * [x0 | nominal | sigma | task params | ctrl bounds] (float offsets o_* into it) into blk_dev, jh_rollout_cost_traced, jh_update_fused with its outputs at
 * out = [nominal K*nu | sigma K*nu | E x (2 + row_floats) trace records] (device memory, or device-visible pinned host memory: then no download is needed), and the
 * completion mark of jh_download_begin (zero bytes).  Asynchronous on `stream`; jh_download_end waits.  `trace` NULL: no trace records (E ignored).
 * Round 6, for plan steps whose kernels are a few tens of microseconds (cartpole, cylinder_push):
 *  - those models run rollout + cost + update as ONE launch (the update's tail inside the rollout kernel's launch: same bits as the two launches);
 *  - blk_dev == blk_host (a device-visible pinned host block): no upload, the kernel reads the block in place;
 *  - out_host_mark != out: a 4-byte word in device-visible pinned host memory; the update's last workgroup stores (its value at the time of this call) + 1 there behind
 *    the results and jh_download_end polls that word instead of waiting for the stream's event (one outstanding plan step per word).  out_host_mark == out: the event. */
int jh_plan_step(const jh_model* m, void* blk_dev, const void* blk_host, size_t blk_bytes, int o_nominal, int o_sigma, int o_tp, int o_lohi, const float* noise, int ldn,
                 const float* W, int phase, int N, int n_offset, int H, int K, float* costs, float* knots_out, float* trace, int mode, float lambda, int k, int tie_high, int E,
                 int row_floats, int colmajor, float* scratch, float* out, void* out_host_mark, void* const* timing, void* stream);
/* B independent plan steps of ONE model in one call and one wait: B controllers (several robots, several goals, a domain-randomised sweep) whose iterations of
 * Controller.update_action's loop (judo/controller/controller.py:250-299) the reference would run back to back, one process and one launch chain each.  jh_plan_step with a
 * leading B and strides; the problems share the model, N, H, K, W, the optimizer kind and the scalar arguments (mode, lambda, k, tie_high, E), and each has its own
 *   packed block   [x0 | nominal | sigma | task params | ctrl bounds], B sub-blocks blk_stride_bytes apart (a multiple of 4, >= blk_bytes), all with the same o_* offsets;
 *   noise          (K * nu, ldn) per problem, noise_stride_floats apart (>= K * nu * ldn);
 *   costs          B x N;     trace   B x (N x row_floats), or NULL (row_floats = H x jh_model_trace_layout out[1], as for jh_plan_step);
 *   scratch        B x jh_update_fused_scratch_floats(N, K, nu) = jh_plan_batch_scratch_floats(B, N, K, nu) floats, ZERO before the first use (every problem's ticket and,
 *                  in word 1 of problem 0's, the batch's; every launch leaves them at zero);
 *   out            B x out_stride_floats (>= 2 * K * nu + E * (2 + row_floats)), each [nominal | sigma | E trace records].
 * blk_dev == blk_host reads the blocks in place; out_host_mark != out is the polled completion word, stored ONCE, behind the last of the B problems (each problem's last
 * workgroup bumps a batch counter behind a fence of its outputs, the one that draws B - 1 stores the word behind a system-scope fence); out_host_mark == out: the stream's
 * event.  One GPU (n_offset = 0), no knots_out.  A problem's costs, nominal, sigma and trace records are bit for bit those of jh_plan_step on its sub-block: the kernels run
 * the single call's code on offset pointers (cartpole, cylinder_push: one launch with blockIdx.y = problem, or two above jh_model_one_launch_max_knots; the leap family:
 * the rollout kernel on the static grid (groups, B) -- the latency mode chosen from B * N rollouts, no persistent queue -- then the batched update tail).  B = 1 takes the same
 * code.  JH_ERR_INVALID: B < 1, B > 65535 (the grid's second dimension), a stride smaller than a block / a noise slice / an output record, a forced one-launch plan step that
 * does not fit.  JH_ERR_UNSUPPORTED: fr3_pick (its phase is a per-problem host decision, judo/tasks/fr3_pick.py:191-223: jh_plan_step_batch_phases below takes one per problem) and the cross-check kernel generations.  The Spot
 * policy tasks, whose iteration is the materialise path, batch through jh_spline_controls_batch / jh_policy_rollout_batch / jh_update_fused_batch below; the sharded and the
 * plugin-reward paths have no batched form. */
size_t jh_plan_batch_scratch_floats(int B, int N, int K, int nu);
int jh_plan_step_batch(const jh_model* m, int B, void* blk_dev, const void* blk_host, size_t blk_bytes, size_t blk_stride_bytes, int o_nominal, int o_sigma, int o_tp, int o_lohi,
                       const float* noise, int ldn, size_t noise_stride_floats, const float* W, int N, int H, int K, float* costs, float* trace, int mode, float lambda, int k,
                       int tie_high, int E, int row_floats, int colmajor, float* scratch, float* out, size_t out_stride_floats, void* out_host_mark, void* const* timing,
                       void* stream);
/* jh_plan_step_batch for fr3_pick: B arms, each in its own phase, in one call and one wait instead of B jh_plan_step calls back to back (the reference's shipped
 * configuration, 64 rollouts x 250 steps, is 16-64 one-wave workgroups per call).  jh_plan_step takes the phase (LIFT / MOVE / PLACE / HOMING, judo/tasks/fr3_pick.py:191-223:
 * a host decision from the controller's own state) as an argument; here it is one more word of every problem's packed block,
 *   packed block   [x0 | nominal | sigma | task params | ctrl bounds | ... phase ...], the phase word at float offset o_phase (4 * (o_phase + 1) <= blk_bytes),
 * a FLOAT holding exactly 0.0, 1.0, 2.0 or 3.0 -- the block is a block of floats everywhere else.  The rollout kernel runs on the grid (groups, B), reads its problem's
 * word once per workgroup with a uniform load and converts it once; the latency mode is chosen from B * N rollouts.  Everything else -- blocks, strides, noise, costs,
 * trace (6 floats per step), scratch, out, the completion mark, timing -- is jh_plan_step_batch's.  Problem b's costs, nominal, sigma and trace records are bit for bit
 * those of jh_plan_step(..., phase_b, ...) on its sub-block; both builds of the fr3 kernel (jh_model_fr3_build) are served.  The counters of jh_model_stats are the model's,
 * whichever problem a rollout belongs to.
 * JH_ERR_UNSUPPORTED: any model that is not fr3_pick (jh_plan_step_batch plans those).  JH_ERR_INVALID: o_phase < 0 or outside the block; a phase word that is not
 * exactly 0, 1, 2 or 3 (read from blk_host before anything is launched; the message names the problem); K > 8; everything jh_plan_step_batch refuses.  jh_plan_step_batch and
 * the model-set, ensemble and randomised entries keep refusing fr3_pick; a model image per problem comes with jh_fr3_model_set_create and
 * jh_plan_step_batch_phases_models below. */
int jh_plan_step_batch_phases(const jh_model* m, int B, void* blk_dev, const void* blk_host, size_t blk_bytes, size_t blk_stride_bytes, int o_nominal, int o_sigma, int o_tp, int o_lohi,
                              int o_phase, const float* noise, int ldn, size_t noise_stride_floats, const float* W, int N, int H, int K, float* costs, float* trace, int mode,
                              float lambda, int k, int tie_high, int E, int row_floats, int colmajor, float* scratch, float* out, size_t out_stride_floats, void* out_host_mark,
                              void* const* timing, void* stream);
/* jh_plan_step_batch with a model image PER PROBLEM (randomised physics: B planners of one task with B cube masses or friction coefficients, a bank of mass hypotheses,
 * one controller over perturbed plants).  The reference has no counterpart.  A model set is B model handles whose FLOAT sections sit in one device buffer, a fixed stride
 * apart; everything else -- the int section (topology, pair lists, lane lists), the dimensions, the kernel build and its settings -- is member 0's and must be the same in
 * every member.  That is what a description perturbed in its masses, inertias, friction coefficients or actuator gains packs to (judo_amd.models.scaled_description).
 *   jh_model_set_create   checks the members (below), then copies their float sections device to device into one allocation on member 0's device; the stride is the float
 *                         count rounded up to a multiple of 64 floats, so every image keeps the alignment a model's own has.  The set keeps models[0] -- which must outlive
 *                         it -- for everything else; the other handles may be destroyed.  Settings (jh_model_set_self_collision, jh_model_set_plan_step_launches ...) are
 *                         read from member 0 at every launch.
 *   jh_model_set_update   replaces member b's image, after the same checks (re-randomising between episodes).  Synchronous; not meant for the plan loop.  b = 0: `model`
 *                         becomes the handle the set keeps.
 *   jh_model_set_info     out[0] = B, out[1] = floats per image, out[2] = the stride in floats, out[3] = members whose image differs from member 0's.
 *   jh_plan_step_batch_models   jh_plan_step_batch without `m` and `B`: the same blocks, noise, costs, trace, scratch and out with the same strides, the same completion mark.
 *                         Problem b runs on image b: its costs, nominal, sigma and trace records are bit for bit those of jh_plan_step on member b's own handle and
 *                         sub-block (the kernels offset the base of the float section by blockIdx.y * stride, scalar arithmetic on kernel arguments, and run the single
 *                         call's code).  jh_plan_step_batch itself is this code path with stride 0.
 * The diagnostic counters of a set launch (jh_model_stats) land in MEMBER 0's handle, whichever problem a rollout belongs to.
 * jh_model_set_create / _update refuse, with jh_last_error naming the member and the field: B < 1 or B > 65535 (JH_ERR_INVALID); a member on another device, or with another
 * kind, nq, nv, nu, ns, ntaskparam, nf or ni; an int section (h_i) that is not byte for byte member 0's; another kernel_gen, contact_capacity, cylinders, self_collision,
 * rollout_schedule or plan_step_launches (all JH_ERR_INVALID); fr3_pick and leap models off kernel generation 3, as jh_plan_step_batch does (JH_ERR_UNSUPPORTED); and a
 * member whose image the kernel's own launcher would refuse -- each image is held to the single call's acceptance test on its own floats, e.g. the leap kernel's isotropic
 * cube inertia (JH_ERR_UNSUPPORTED). */
typedef struct jh_model_set jh_model_set;
int jh_model_set_create(const jh_model* const* models /* HOST array of B handles */, int B, jh_model_set** out);
int jh_model_set_update(jh_model_set* set, int b, const jh_model* model);
int jh_model_set_info(const jh_model_set* set, int* out /* HOST, 4 ints */);
void jh_model_set_destroy(jh_model_set* set);
/* A model set of fr3_pick models (pick-and-place under an unknown cube mass, pad friction or gripper gain).  jh_model_set_create keeps refusing the family, because the
 * five entries above and below that take its sets carry no phase; this constructor makes the same record for fr3_pick members alone, and the entries that carry a
 * phase plan it -- the two here and the three `_phase` / `_phases` forms of the ensemble and randomised entries below:
 *   jh_fr3_model_set_create            the checks of jh_model_set_create member by member -- the same fields, arm_pairs among them, so the default and the self-collision
 *                                      build do not mix; each image must pass its own build's acceptance test on its own floats (the finger slides antiparallel).
 *                                      JH_ERR_UNSUPPORTED for a member that is no fr3_pick model.  jh_model_set_update, _info and _destroy work on the set; _update refuses an
 *                                      fr3_pick member for any other set and any other member for this one (JH_ERR_UNSUPPORTED).  fr3_pick images hold no pair tables
 *                                      (jh_model_set_pair_tables: 0), and the launches read member 0's int section as it is.
 *   jh_plan_step_batch_phases_models   jh_plan_step_batch_phases with the set in place of the model: B must be the set's size (JH_ERR_INVALID otherwise), problem b runs on
 *                                      image b with the phase word of its block, and its costs, nominal, sigma and trace records are bit for bit those of
 *                                      jh_plan_step(member b's own handle, ..., phase_b, ...) on its sub-block.  The kernel offsets the base of the float section by
 *                                      blockIdx.y * stride, scalar arithmetic on kernel arguments; jh_plan_step_batch_phases is this code path with stride 0.
 *                                      JH_ERR_UNSUPPORTED: a set of any other family (jh_plan_step_batch_models plans those).
 *   jh_plan_step_randomized_phase      jh_plan_step_randomized (below) with `phase`, 0..3, behind W: one arm in one phase, its N candidates in G blocks of N / G, block g
 *                                      on plant plant_of_block[g].  costs[r] is bit for bit costs[r] of jh_plan_step(handle of plant plant_of_block[r / Nb], ..., phase, ...)
 *                                      with the same block and noise; only global rollout 0 is noise-free; out = nominal | sigma is what jh_update_fused writes for the
 *                                      N costs.  No trace buffer.  Every check of jh_plan_step_randomized, plus JH_ERR_INVALID for a phase outside 0..3 and K > 8 and
 *                                      JH_ERR_UNSUPPORTED for a set that is not fr3_pick, all before anything is enqueued.
 * The fr3 launch has a controller axis in blockIdx.z, as the leap kernel's has, and three more entries use it for an fr3 set (documented with the entries they extend,
 * below): jh_plan_step_ensemble_phase, jh_plan_step_ensemble_batch_phases and jh_plan_step_randomized_batch_phases.  jh_plan_step_ensemble, _ensemble_batch,
 * _randomized, _randomized_batch and jh_plan_step_batch_models carry no phase and keep refusing an fr3 set (JH_ERR_UNSUPPORTED), naming the entries that serve it. */
int jh_fr3_model_set_create(const jh_model* const* models /* HOST array of B handles */, int B, jh_model_set** out);
int jh_plan_step_batch_phases_models(const jh_model_set* set, int B, void* blk_dev, const void* blk_host, size_t blk_bytes, size_t blk_stride_bytes, int o_nominal, int o_sigma, int o_tp,
                                     int o_lohi, int o_phase, const float* noise, int ldn, size_t noise_stride_floats, const float* W, int N, int H, int K, float* costs, float* trace,
                                     int mode, float lambda, int k, int tie_high, int E, int row_floats, int colmajor, float* scratch, float* out, size_t out_stride_floats,
                                     void* out_host_mark, void* const* timing, void* stream);
int jh_plan_step_randomized_phase(const jh_model_set* set, void* blk_dev, const void* blk_host, size_t blk_bytes, int o_nominal, int o_sigma, int o_tp, int o_lohi, const float* noise, int ldn,
                                  const float* W, int phase, int N, int H, int K, const unsigned char* plant_of_block /* HOST, G */, int G, float* costs /* DEVICE, N */, int mode,
                                  float lambda, int k, int tie_high, float* scratch, float* out /* nominal | sigma */, void* out_host_mark, void* const* timing, void* stream);

/* The hand's pair tables (leap family; judo_amd/engine_model.py::hand_pair_tables): bit grids over two joint angles in the image's int section that tell the kernel which
 * hand body pairs cannot touch at a step's pose.  jh_model_create refuses a malformed block (JH_ERR_BLOB).  A model set reads ONE int section, member 0's, so it keeps the
 * tables only while every member agrees with member 0 on the tables and on everything they were computed from -- the hand bodies' frames, joint axes and ranges, the hand
 * geoms' sizes and poses, the bodies' bounding volumes; members that differ only in the cube, masses, gains or friction keep them.  Otherwise the set's launches read a
 * copy of the int section without tables (the same results, every pair tested).
 * The two entry points below are DIAGNOSTIC: they report what the library decided and change nothing; tests and tools/diag use them.  (So is the description key
 * "pair_tables": false, which packs an image without tables.)
 *   jh_model_set_pair_tables   1: the set's launches use the tables, 0: they do not (or the images have none).
 *   jh_pair_tables_shared      the same rule on two packed blobs, without a device: 1 if a set of the two keeps blob0's tables, 0 if not; negative: not a model blob. */
int jh_model_set_pair_tables(const jh_model_set* set);
int jh_pair_tables_shared(const void* blob0, size_t nbytes0, const void* blob, size_t nbytes);
int jh_plan_step_batch_models(const jh_model_set* set, void* blk_dev, const void* blk_host, size_t blk_bytes, size_t blk_stride_bytes, int o_nominal, int o_sigma, int o_tp, int o_lohi,
                              const float* noise, int ldn, size_t noise_stride_floats, const float* W, int N, int H, int K, float* costs, float* trace, int mode, float lambda, int k,
                              int tie_high, int E, int row_floats, int colmajor, float* scratch, float* out, size_t out_stride_floats, void* out_host_mark, void* const* timing,
                              void* stream);
/* ONE plan step against an ensemble of plants (sim-to-real: one controller with one nominal spline over M perturbed models; the reference has no counterpart).  The N
 * candidates of one packed block and one noise slice are rolled out on every member of a model set, M <= JH_MAX_ENSEMBLE, and a candidate's cost is a risk measure over
 * its M member costs c[0..M-1], fixed here so that it can be tested bit for bit: with `worst` = j, 1 <= j <= M,
 *   take the j largest values as a multiset (equal values are interchangeable), add them in fp32 in DESCENDING order starting from the largest (acc = v0; acc += v1; ...),
 *   then cost = acc / (float)j, a correctly rounded fp32 division.
 * j = 1 is the exact maximum (the worst case), j = M the mean, in between the mean of the worst j, a tail mean that stands in for CVaR.  +inf and the 3.0e38 sentinel behave
 * as IEEE arithmetic makes them (3.0e38 + 3.0e38 = +inf); NaN member costs are outside the contract.  judo_amd/ensemble.py::aggregate_costs_host restates it in numpy.
 *   jh_ensemble_costs       the aggregation alone: member m's cost of rollout r at member_costs[m * ld + r] (ld >= N; what lies between N and ld is not read), costs[0..N-1]
 *                           written.  JH_ERR_INVALID, with jh_last_error naming the argument: a null pointer, M outside 1..JH_MAX_ENSEMBLE, N < 1, ld < N, worst outside 1..M.
 *   jh_plan_step_ensemble   jh_plan_step on the set: one upload of the block (blk_dev == blk_host: read in place), the batched rollout kernel on the grid (workgroups, M) with the
 *                           members sharing the block and the noise -- member b's costs land in member_costs[b * N ..] and are bit for bit those of jh_plan_step on member b's
 *                           own handle --, then ONE launch that writes the aggregated costs into `costs` and runs the update's tail on them: out = [nominal K*nu | sigma K*nu]
 *                           is bit for bit what jh_update_fused writes for those costs.  Two launches for every model; no trace buffer and no knots_out (the caller re-rolls its
 *                           trace elites on the member it calls nominal).  One completion mark, as for jh_plan_step: out_host_mark == out is the stream's event, anything else the
 *                           polled 4-byte word.  scratch: jh_update_fused_scratch_floats(N, K, nu) floats, ZERO before the first use; every launch leaves the ticket at zero.
 *                           M = 1 takes the same code.  The diagnostic counters land in member 0's handle.  JH_ERR_INVALID, naming the argument: a null pointer, a set of more than
 *                           JH_MAX_ENSEMBLE members, worst outside 1..M, N, H or K < 1, ldn < N, K * nu > JH_MAX_KNOT_DIM, a negative offset or a block too small for them, a bad
 *                           mode / lambda / k, and a member 0 whose plan step is forced to one launch.  JH_ERR_UNSUPPORTED: as jh_plan_step_batch (a set holds neither fr3_pick
 *                           nor a cross-check generation when it is made; a later change of member 0's kernel generation is caught here). */
int jh_ensemble_costs(const float* member_costs /* DEVICE, M x ld */, int M, int N, int ld, int worst, float* costs /* DEVICE, N */, void* stream);
int jh_plan_step_ensemble(const jh_model_set* set, void* blk_dev, const void* blk_host, size_t blk_bytes, int o_nominal, int o_sigma, int o_tp, int o_lohi, const float* noise, int ldn,
                          const float* W, int N, int H, int K, float* member_costs /* DEVICE, M x N */, float* costs /* DEVICE, N */, int worst, int mode, float lambda, int k,
                          int tie_high, float* scratch, float* out /* nominal | sigma */, void* out_host_mark, void* const* timing, void* stream);
/* jh_plan_step_ensemble for fr3_pick, with `phase`, 0..3, behind W: one arm in one phase against the M plants of an fr3 set (jh_fr3_model_set_create).  The fr3 kernel's
 * batched launch on the grid (workgroups, M): every member takes the phase from the launch record as the single launch takes its argument, so row m of member_costs is
 * bit for bit the costs of jh_plan_step(member m's own handle, ..., phase, ...) with the same block and noise; `costs` and out = nominal | sigma are the ensemble call's.
 * The latency mode is chosen from the M * N rollouts of the launch (the bits do not depend on it).  Every check of jh_plan_step_ensemble, plus JH_ERR_INVALID for a phase
 * outside 0..3 and K > 8 and JH_ERR_UNSUPPORTED for a set that is not fr3_pick (jh_plan_step_ensemble plans those), all before anything is enqueued. */
int jh_plan_step_ensemble_phase(const jh_model_set* set, void* blk_dev, const void* blk_host, size_t blk_bytes, int o_nominal, int o_sigma, int o_tp, int o_lohi, const float* noise, int ldn,
                                const float* W, int phase, int N, int H, int K, float* member_costs /* DEVICE, M x N */, float* costs /* DEVICE, N */, int worst, int mode, float lambda, int k,
                                int tie_high, float* scratch, float* out /* nominal | sigma */, void* out_host_mark, void* const* timing, void* stream);
/* The plant-weighted risk measure: the tail mean (CVaR) of a candidate's member costs c[0..M-1] under fp32 weights p[0..M-1] (each finite and >= 0, at least one > 0; a
 * posterior over the plants, judo_amd/identify.py) with the tail mass `tail`, fp32 in (0, 1].  Fixed here so that it can be tested bit for bit:
 *   got = 0.  Visit the DISTINCT values of c in strictly descending order.  For a value v: ws is the sum of the weights of the members with c[m] == v, taken in ascending
 *   m and starting from the first (ws = p[m0]; ws = ws + p[m1]; ...); take = min(ws, tail - got).  If take > 0: t = take * v; acc = t for the first such term, else
 *   acc = acc + t; got = got + take.  A group with take == 0 contributes nothing (a +inf member of weight zero makes no NaN).  Stop when got >= tail or the values are
 *   exhausted.  cost = acc / got.
 * Every product, sum, difference and quotient is rounded to fp32 on its own; no fused multiply-add.  The divisor is the mass actually taken, so weights that add up to
 * less than `tail` give the weighted mean of everything, and the weights need not add up to 1.  +inf and the 3.0e38 sentinel behave as IEEE arithmetic makes them; NaN
 * member costs are outside the contract.  One-hot weights with tail = 1 return that member's costs exactly; uniform weights 1 / M with tail = j / M, M a power of two, are
 * bit for bit `worst` = j on a rollout whose M costs are pairwise distinct (with ties 3 * v is rounded once and v + v + v twice).
 * judo_amd/ensemble.py::aggregate_costs_weighted_host restates it in numpy.
 *   jh_ensemble_costs_weighted            jh_ensemble_costs with `weights` (HOST, M floats, read before the call returns: they travel in the kernel arguments) and `tail`
 *                                         where `worst` stands.  JH_ERR_INVALID, naming the argument: what jh_ensemble_costs refuses, null `weights`, a weight that is
 *                                         negative or not finite (the index is named), all weights zero, `tail` outside (0, 1] or NaN.
 *   jh_plan_step_ensemble_weighted        jh_plan_step_ensemble with `weights` and `tail` where `worst` stands: the same rollout launch, so member_costs are bit for bit the
 *                                         unweighted entry's; the tail launch aggregates with the weighted measure and updates.  Following a belief between plan steps
 *                                         costs no copy and no launch.  Every check of jh_plan_step_ensemble but `worst`'s, and those of the weights and the tail above,
 *                                         all before anything is enqueued.
 *   jh_plan_step_ensemble_weighted_phase  the same for fr3_pick, `phase` behind W: the rules of jh_plan_step_ensemble_phase.
 * The batched entries take the measure per controller from a risk record in the controller's packed block (jh_plan_step_ensemble_batch_risk, below): B x M weights do
 * not fit in the kernel arguments. */
int jh_ensemble_costs_weighted(const float* member_costs /* DEVICE, M x ld */, int M, int N, int ld, const float* weights /* HOST, M */, float tail, float* costs /* DEVICE, N */,
                               void* stream);
int jh_plan_step_ensemble_weighted(const jh_model_set* set, void* blk_dev, const void* blk_host, size_t blk_bytes, int o_nominal, int o_sigma, int o_tp, int o_lohi, const float* noise,
                                   int ldn, const float* W, int N, int H, int K, float* member_costs /* DEVICE, M x N */, float* costs /* DEVICE, N */,
                                   const float* weights /* HOST, M */, float tail, int mode, float lambda, int k, int tie_high, float* scratch, float* out /* nominal | sigma */,
                                   void* out_host_mark, void* const* timing, void* stream);
int jh_plan_step_ensemble_weighted_phase(const jh_model_set* set, void* blk_dev, const void* blk_host, size_t blk_bytes, int o_nominal, int o_sigma, int o_tp, int o_lohi,
                                         const float* noise, int ldn, const float* W, int phase, int N, int H, int K, float* member_costs /* DEVICE, M x N */,
                                         float* costs /* DEVICE, N */, const float* weights /* HOST, M */, float tail, int mode, float lambda, int k, int tie_high, float* scratch,
                                         float* out /* nominal | sigma */, void* out_host_mark, void* const* timing, void* stream);
/* B ensemble plan steps as ONE call with ONE completion mark (several robots, or one robot swept over risk levels, goals or seeds: B controllers that each plan against
 * M plants; the reference has no counterpart).  Controller b rolls its own N candidates out on its M plants, aggregates them with its own worst[b] and updates its own
 * nominal; its results are bit for bit those of jh_plan_step_ensemble on its block, its noise and its plants with worst[b].
 *   per controller   the packed block x0 | nominal | sigma | task params | bounds, blk_stride_bytes apart; the noise, noise_stride_floats apart; the update scratch,
 *                    jh_update_fused_scratch_floats(N, K, nu) floats apart (jh_plan_batch_scratch_floats(B, N, K, nu) in all, ZERO before the first use: the B + 1 ticket
 *                    words, which every launch leaves at zero); the output record nominal K*nu | sigma K*nu, out_stride_floats apart; the row b of `costs` (B x N); the slab
 *                    b of `member_costs` (B x M x N, controller-major: plant m's cost of controller b's rollout r at (b * M + m) * N + r); worst[b]
 *   shared           N, H, K, W, mode, lambda, k, tie_high; no trace buffer and no knots_out, as for the ensemble call
 *   the plants       a set of M members, which every controller plans against, or a set of B * M members, controller-major: member b * M + m is controller b's plant m.
 *                    M <= JH_MAX_ENSEMBLE, B <= JH_MAX_ENSEMBLE_FLEET.  A set of any other size: JH_ERR_INVALID with the three numbers
 *   worst            a HOST array of B ints, each in 1..M (the error names the controller), read before the call returns: the values travel in the kernel arguments
 * Two launches for every model: the batched rollout kernel on the grid (workgroups, M, B) -- the leap kernel's latency mode is chosen from the B * M * N rollouts of the
 * launch, and the bits do not depend on it; no queue --, then the aggregation and the update's tail on (tail workgroups, B) with the two-level ticket of
 * jh_plan_step_batch.  The completion mark is that call's: out_host_mark == out is the stream's event, anything else the polled 4-byte word, which receives its old value
 * + 1 behind the last controller's results.  B = 1 and M = 1 take the same code.  Everything is checked before anything is enqueued.  JH_ERR_INVALID, naming the
 * argument: what jh_plan_step_ensemble refuses (each null pointer by name, `worst` included), B or M outside their limits, a stride smaller than a block / a noise slice
 * / an output record, a member 0 whose plan step is forced to one launch.  JH_ERR_UNSUPPORTED: as jh_plan_step_ensemble. */
int jh_plan_step_ensemble_batch(const jh_model_set* set, int B, int M, void* blk_dev, const void* blk_host, size_t blk_bytes, size_t blk_stride_bytes, int o_nominal, int o_sigma, int o_tp,
                                int o_lohi, const float* noise, int ldn, size_t noise_stride_floats, const float* W, int N, int H, int K, float* member_costs /* DEVICE, B x M x N */,
                                float* costs /* DEVICE, B x N */, const int* worst /* HOST, B */, int mode, float lambda, int k, int tie_high, float* scratch, float* out, size_t out_stride_floats,
                                void* out_host_mark, void* const* timing, void* stream);
/* jh_plan_step_ensemble_batch for fr3_pick, with `o_phase` behind o_lohi as in jh_plan_step_batch_phases: controller c's phase is the float word at offset o_phase of its
 * own packed block (0.0, 1.0, 2.0 or 3.0), which its M members all read -- the members' block stride is 0, the controller's is blk_stride_bytes.  The fr3 kernel's batched
 * launch on the grid (workgroups, M, B); controller c's results are bit for bit those of jh_plan_step_ensemble_phase on its block, noise and plants with worst[c] and its
 * phase.  The set is shared (M plants) or per controller (B * M), as above.  Every check of jh_plan_step_ensemble_batch, plus JH_ERR_INVALID for an o_phase that is negative
 * or outside the block, for a phase word that is not exactly 0, 1, 2 or 3 (read from the HOST block; the error names the controller) and for K > 8, and
 * JH_ERR_UNSUPPORTED for a set that is not fr3_pick (jh_plan_step_ensemble_batch plans those), all before anything is enqueued. */
int jh_plan_step_ensemble_batch_phases(const jh_model_set* set, int B, int M, void* blk_dev, const void* blk_host, size_t blk_bytes, size_t blk_stride_bytes, int o_nominal, int o_sigma, int o_tp,
                                       int o_lohi, int o_phase, const float* noise, int ldn, size_t noise_stride_floats, const float* W, int N, int H, int K,
                                       float* member_costs /* DEVICE, B x M x N */, float* costs /* DEVICE, B x N */, const int* worst /* HOST, B */, int mode, float lambda, int k, int tie_high,
                                       float* scratch, float* out, size_t out_stride_floats, void* out_host_mark, void* const* timing, void* stream);
/* B ensemble plan steps in one call, each controller under a risk measure of its own: counted (`worst`) or plant-weighted, chosen per controller and per plan step.  With
 * B <= JH_MAX_ENSEMBLE_FLEET and M <= JH_MAX_ENSEMBLE the weights are up to 32 KB and cannot travel by value, so they travel where fr3_pick's phase word does: in words of the
 * controller's own packed block, behind its five sections, which go up with the block upload that happens anyway or are read in place with the block.
 *   the risk record  1 + M fp32 words at the float offset `o_risk` of every controller's block (the same offset for all):
 *                      the tail word   exactly 0.0: the counted measure with worst[b], as in jh_plan_step_ensemble_batch (the weights are not read); any other value is
 *                                      the tail mass of the weighted measure and lies in (0, 1].  NaN, negative values and values above 1 are refused.
 *                      the M weights   each finite and >= 0, at least one > 0; read only where the tail word is not zero.
 *   the cost         a weighted controller's aggregated cost is, word for word, the definition above jh_ensemble_costs_weighted with its record's weights and tail; an
 *                    unweighted controller's is jh_ensemble_costs' with worst[b].  Nothing new is defined, only where the parameters come from.
 *   jh_ensemble_costs_risk_batch          the aggregation alone for B controllers: plant m's cost of controller b's rollout r at member_costs[(b * M + m) * ld + r] (ld >= N;
 *                                         what lies between N and ld is not read), controller b's record at risk[b * risk_stride_floats ..] (risk_stride_floats >= 1 + M;
 *                                         the words behind 1 + M are not read), costs[b * ldc + r] written (ldc >= N; what lies between N and ldc is not written).  The
 *                                         records are DEVICE memory here, so the entry checks what it can before the enqueue -- each pointer, B in 1..JH_MAX_ENSEMBLE_FLEET,
 *                                         M in 1..JH_MAX_ENSEMBLE, N >= 1, ld >= N, ldc >= N, the stride, every worst[b] in 1..M (HOST, B ints), JH_ERR_INVALID naming
 *                                         the argument -- and NOT the records' contents: a record outside the rules above is outside the contract.
 *   jh_plan_step_ensemble_batch_risk      jh_plan_step_ensemble_batch with `o_risk` behind o_lohi.  The rollout launch is the same call, so member_costs are bit for bit the
 *                                         unweighted batched entry's; the tail on (tail workgroups, B) reads its controller's record as wave-uniform loads and aggregates
 *                                         with the measure it names.  Controller b's costs and output record are bit for bit jh_plan_step_ensemble_weighted's with its
 *                                         weights and tail, or jh_plan_step_ensemble's with worst[b] where its tail word is 0.0; with every tail word 0.0 the call equals
 *                                         jh_plan_step_ensemble_batch in every output.  New records for the next plan step cost no copy and no launch of their own.
 *                                         Every check before the first enqueue, JH_ERR_INVALID naming the argument: everything jh_plan_step_ensemble_batch refuses; worst[b]
 *                                         outside 1..M for every b, weighted or not; o_risk negative; o_risk + 1 + M beyond blk_bytes / 4 (blk_bytes must cover the record:
 *                                         the upload copies (B - 1) * blk_stride_bytes + blk_bytes); a record that overlaps x0, nominal, sigma, the task params, the bounds
 *                                         or the phase word; and, read from the HOST block, a tail word that is NaN, negative or above 1 (the controller is named), a weight
 *                                         that is negative or not finite (controller and index named), all weights zero (controller named).  JH_ERR_UNSUPPORTED as
 *                                         jh_plan_step_ensemble_batch: an fr3_pick set is refused, and the error names the phase entry.
 *   jh_plan_step_ensemble_batch_phases_risk  jh_plan_step_ensemble_batch_phases with `o_risk` behind o_phase: the same rules; any set but fr3_pick's is JH_ERR_UNSUPPORTED. */
int jh_ensemble_costs_risk_batch(const float* member_costs /* DEVICE, B x M x ld */, int B, int M, int N, int ld, const float* risk /* DEVICE, B records */, size_t risk_stride_floats,
                                 const int* worst /* HOST, B */, float* costs /* DEVICE, B x ldc */, int ldc, void* stream);
int jh_plan_step_ensemble_batch_risk(const jh_model_set* set, int B, int M, void* blk_dev, const void* blk_host, size_t blk_bytes, size_t blk_stride_bytes, int o_nominal, int o_sigma, int o_tp,
                                     int o_lohi, int o_risk, const float* noise, int ldn, size_t noise_stride_floats, const float* W, int N, int H, int K,
                                     float* member_costs /* DEVICE, B x M x N */, float* costs /* DEVICE, B x N */, const int* worst /* HOST, B */, int mode, float lambda, int k, int tie_high,
                                     float* scratch, float* out, size_t out_stride_floats, void* out_host_mark, void* const* timing, void* stream);
int jh_plan_step_ensemble_batch_phases_risk(const jh_model_set* set, int B, int M, void* blk_dev, const void* blk_host, size_t blk_bytes, size_t blk_stride_bytes, int o_nominal, int o_sigma,
                                            int o_tp, int o_lohi, int o_phase, int o_risk, const float* noise, int ldn, size_t noise_stride_floats, const float* W, int N, int H, int K,
                                            float* member_costs /* DEVICE, B x M x N */, float* costs /* DEVICE, B x N */, const int* worst /* HOST, B */, int mode, float lambda, int k,
                                            int tie_high, float* scratch, float* out, size_t out_stride_floats, void* out_host_mark, void* const* timing, void* stream);
/* ONE domain-randomised plan step (MPPI / CEM / PS with a plant drawn per rollout; the reference has no counterpart): one controller, one nominal spline, N candidates,
 * each rolled out on ONE member of a model set, M <= JH_MAX_ENSEMBLE, and the update on the N costs as they are -- the rollouts of a plain plan step, never fitted to one
 * plant.  The rule, fixed here so that it can be tested bit for bit: the N candidates form G contiguous blocks of Nb = N / G rollouts (N % G == 0), block g is rollouts
 * [g * Nb, (g + 1) * Nb) and runs on plant plant_of_block[g], 0 <= plant < M.  1 <= G <= JH_MAX_PLANT_BLOCKS; G may exceed M, and a plant named by several blocks carries
 * that share of the candidates (this is how weights are expressed); G = 1 is a plain plan step on that plant.
 *   costs            the cost of rollout r is bit for bit costs[r] of jh_plan_step on the handle of plant plant_of_block[r / Nb] with the same block, noise (pitch ldn,
 *                    column r), W, N, H and K
 *   noise            global rollout 0 is the noise-free nominal, as everywhere else; the first rollout of every later block carries its noise
 *   update           out = [nominal K*nu | sigma K*nu] is bit for bit what jh_update_fused writes for those N costs
 *   plant_of_block   a HOST array of G bytes, read before the call returns: the values travel in the kernel arguments, so another assignment for the next plan step costs
 *                    no copy and no launch
 * Two launches for every model, as for jh_plan_step_ensemble: the batched rollout kernel on the grid (workgroups of Nb rollouts, G) -- the block stride 0, the noise, cost
 * and rollout-index strides Nb, the image from the table; the leap kernel's latency mode is chosen from the N rollouts of the launch, as the single call chooses it; no queue
 * and no horizon slices --, then the one-problem update tail on `costs`.  The completion mark, the scratch (jh_update_fused_scratch_floats(N, K, nu) floats, ZERO before the
 * first use; every launch leaves the ticket at zero), the int section and the counters (member 0's handle) are jh_plan_step_ensemble's; no trace buffer and no knots_out.
 * Everything is checked before anything is enqueued.  JH_ERR_INVALID, with jh_last_error naming the argument: what jh_plan_step_ensemble refuses (each null pointer by
 * name, plant_of_block included), G outside 1..JH_MAX_PLANT_BLOCKS, N % G != 0, an entry of the table >= M (named with its block).  JH_ERR_UNSUPPORTED: as
 * jh_plan_step_ensemble. */
int jh_plan_step_randomized(const jh_model_set* set, void* blk_dev, const void* blk_host, size_t blk_bytes, int o_nominal, int o_sigma, int o_tp, int o_lohi, const float* noise, int ldn,
                            const float* W, int N, int H, int K, const unsigned char* plant_of_block /* HOST, G */, int G, float* costs /* DEVICE, N */, int mode, float lambda, int k,
                            int tie_high, float* scratch, float* out /* nominal | sigma */, void* out_host_mark, void* const* timing, void* stream);
/* B domain-randomised plan steps as ONE call with ONE completion mark (several robots, or one robot swept over seeds, goals or plant weights: B controllers that each
 * spread their N candidates over the plants of a set; the reference has no counterpart).  Controller b's results -- its row of `costs` and its record nominal | sigma --
 * are bit for bit what jh_plan_step_randomized writes on b's block, b's noise slice and b's plants with the table plant_of_block[b * G .. b * G + G).
 *   per controller   the packed block x0 | nominal | sigma | task params | bounds, blk_stride_bytes apart; the noise, noise_stride_floats apart; the update scratch,
 *                    jh_update_fused_scratch_floats(N, K, nu) floats apart (jh_plan_batch_scratch_floats(B, N, K, nu) in all, ZERO before the first use: the B + 1 ticket
 *                    words, which every launch leaves at zero); the output record nominal K*nu | sigma K*nu, out_stride_floats apart; the row b of `costs` (B x N); its G
 *                    bytes of the table
 *   shared           N, H, K, G, W, mode, lambda, k, tie_high; no trace buffer and no knots_out, as for the randomised call
 *   the plants       a set of M members, which every controller shares, or a set of B * M members, controller-major: member b * M + m is controller b's plant m.
 *                    M <= JH_MAX_ENSEMBLE.  A set of any other size: JH_ERR_INVALID with the three numbers
 *   plant_of_block   a HOST array of B x G bytes, controller-major, each < M, read before the call returns: the values travel in the kernel arguments, so a re-drawn
 *                    assignment costs no copy and no launch.  G is a grid dimension and therefore one for the launch
 *   limits           1 <= B <= JH_MAX_ENSEMBLE_FLEET, 1 <= G <= JH_MAX_PLANT_BLOCKS, B * G <= JH_MAX_FLEET_PLANT_BLOCKS (the bytes of the table in the kernel arguments)
 * Two launches for every model: the batched rollout kernel on the grid (workgroups of Nb = N / G rollouts, G, B) -- block stride 0 on y and the controller's on z; noise,
 * cost and rollout-index strides Nb on y; the image from the table entry (controller, block), plus the controller's image stride where the set has B * M members; every
 * controller's global rollout 0 is its noise-free nominal and the first rollout of its later blocks keeps its noise; the leap kernel's latency mode is chosen from the
 * B * N rollouts of the launch, and the bits do not depend on it; no queue and no horizon slices --, then the update's tail on (tail workgroups, B) with the two-level
 * ticket of jh_plan_step_batch.  The completion mark is that call's: out_host_mark == out is the stream's event, anything else the polled 4-byte word, which receives
 * its old value + 1 behind the last controller's results.  B = 1 and G = 1 take the same code.  Everything is checked before anything is enqueued.  JH_ERR_INVALID,
 * naming the argument: each null pointer by name (plant_of_block included); B, G, M or B * G outside their limits; N % G != 0; an entry of the table >= M (named with
 * its controller and block); a stride smaller than a block / a noise slice / an output record; a member 0 whose plan step is forced to one launch; what
 * jh_plan_step_randomized refuses otherwise.  JH_ERR_UNSUPPORTED: as jh_plan_step_randomized. */
int jh_plan_step_randomized_batch(const jh_model_set* set, int B, int M, void* blk_dev, const void* blk_host, size_t blk_bytes, size_t blk_stride_bytes, int o_nominal, int o_sigma, int o_tp,
                                  int o_lohi, const float* noise, int ldn, size_t noise_stride_floats, const float* W, int N, int H, int K,
                                  const unsigned char* plant_of_block /* HOST, B x G */, int G, float* costs /* DEVICE, B x N */, int mode, float lambda, int k, int tie_high, float* scratch,
                                  float* out, size_t out_stride_floats, void* out_host_mark, void* const* timing, void* stream);
/* jh_plan_step_randomized_batch for fr3_pick, with `o_phase` behind o_lohi: controller c's phase is the float word at offset o_phase of its own packed block, under the
 * rules of jh_plan_step_ensemble_batch_phases.  The fr3 kernel's batched launch on the grid (workgroups of Nb rollouts, G, B); controller c's row of `costs` and its
 * record are bit for bit what jh_plan_step_randomized_phase writes on c's block, noise slice and plants with its table and its phase, and only each controller's global
 * rollout 0 is noise-free.  Every check of jh_plan_step_randomized_batch, plus the phase-word checks and K > 8 (JH_ERR_INVALID) and JH_ERR_UNSUPPORTED for a set that
 * is not fr3_pick (jh_plan_step_randomized_batch plans those), all before anything is enqueued. */
int jh_plan_step_randomized_batch_phases(const jh_model_set* set, int B, int M, void* blk_dev, const void* blk_host, size_t blk_bytes, size_t blk_stride_bytes, int o_nominal, int o_sigma,
                                         int o_tp, int o_lohi, int o_phase, const float* noise, int ldn, size_t noise_stride_floats, const float* W, int N, int H, int K,
                                         const unsigned char* plant_of_block /* HOST, B x G */, int G, float* costs /* DEVICE, B x N */, int mode, float lambda, int k, int tie_high,
                                         float* scratch, float* out, size_t out_stride_floats, void* out_host_mark, void* const* timing, void* stream);
/* The noise of those B problems in one launch (judo/optimizers/{mppi.py:52,ps.py:43,cem.py:67}, one np.random.randn per controller): problem b's (rows, ldn) slice of `out`
 * (B x rows x ldn floats) is bit for bit what jh_noise_normal(seeds[b], draws[b], rows, 0, n_local, out + b * rows * ldn, ldn) writes; columns n_local .. ldn - 1 are left
 * alone.  seeds / draws: HOST arrays of B entries, read before the call returns (one launch per 256 problems: the pairs travel as kernel arguments). */
int jh_noise_normal_batch(int B, const unsigned long long* seeds /* HOST */, const unsigned int* draws /* HOST */, int rows, int n_local, float* out, int ldn, void* stream);
/* The materialise path of those B problems where the rollout is not a jh_model's (the Spot policy tasks: judo/controller/controller.py:239-299 with
 * judo/utils/policy_mj_rollout_backend.py:60-125 as the rollout), one launch per stage instead of B:
 * jh_spline_controls_batch = jh_spline_controls for B problems (judo/controller/controller.py:239-249, the candidate splines at the rollout times, once per controller): the knots
 * are recomputed as clip(nominal + sigma * noise) from problem b's nominal | sigma | ctrl bounds at the float offsets o_* of its sub-block of `blk` (B sub-blocks
 * blk_stride_floats apart) and its (K * nu, ldn) noise (noise_stride_floats apart); every problem's rollout 0 is its nominal.  controls is (B * N, H, nu), problem-major;
 * problem b's N rows are bit for bit those of jh_spline_controls on its sub-block (the same LDS-staged or global-memory form, chosen from H, K, nu as there).
 * JH_ERR_INVALID: B < 1, B > 65535, a stride smaller than a block (the end of the furthest of the three parts) or than a noise slice (K * nu * ldn). */
int jh_spline_controls_batch(const float* W, int B, const float* blk, size_t blk_stride_floats, int o_nominal, int o_sigma, int o_lohi, const float* noise, int ldn,
                             size_t noise_stride_floats, int N, int H, int K, int nu, float* controls, void* stream);
/* jh_update_fused for B problems whose costs are given (Optimizer.update_nominal_knots and update_traces, judo/controller/controller.py:283-299, once per controller): costs is
 * B x N; nominal | sigma | ctrl bounds and the noise as for jh_spline_controls_batch; trace B x (N x row_floats) or NULL (then E is ignored: the Spot tasks take their traces
 * from the materialised sensors); scratch jh_plan_batch_scratch_floats(B, N, K, nu) floats, ZERO before the first use (the B + 1 tickets, which every launch leaves at zero);
 * out B records [nominal K*nu | sigma K*nu | E x (2 + row_floats) trace records], out_stride_floats apart, in device memory or device-visible pinned host memory, behind ONE
 * completion mark that jh_download_end waits for: out_host_mark == out is the stream's event, anything else a 4-byte word in device-visible pinned host memory that receives
 * its old value + 1 behind the last problem's results (both as for jh_plan_step_batch, whose update stage this is).  Problem b's record is bit for bit what jh_update_fused
 * writes for its costs, sub-block and noise.  JH_ERR_INVALID: B < 1, B > 65535, a stride smaller than a block / a noise slice / an output record. */
int jh_update_fused_batch(int B, const float* costs, const float* blk, size_t blk_stride_floats, int o_nominal, int o_sigma, int o_lohi, const float* noise, int ldn,
                          size_t noise_stride_floats, int N, int K, int nu, int mode, float lambda, int k, int tie_high, int E, const float* trace, int row_floats, int colmajor,
                          float* scratch, float* out, size_t out_stride_floats, void* out_host_mark, void* stream);
/* The same iteration with the rollouts sharded over G ranks (the reference has no multi-process form: judo/controller/controller.py:246-299 runs in one
 * process): launch -> all-gather -> merge.  jh_update_shard is jh_update_fused with the last stage left to the ranks' merge: it writes this rank's record
 *   [ MPPI: beta, S, V(K*nu)  |  elites: k x (cost, global index (bits), knots(K*nu)) ]  followed by  E x (cost, global index (bits), trace row(row_floats))
 * (jh_shard_record_floats floats) into rec_out; jh_shard_merge takes the G all-gathered records (rank-major) and writes nominal_out / sigma_out (raw population
 * std, may be NULL) / trace_out (the E best of the G * E trace records, best first, ties: higher index first) exactly as jh_update_fused does on one GPU.  Every rank
 * runs the same merge on the same bytes: identical nominal everywhere, no broadcast.  jh_plan_step_shard = upload + jh_rollout_cost_traced + jh_update_shard in one
 * call (timing: 3 events as for jh_plan_step); jh_plan_merge = jh_shard_merge into out = [nominal | sigma | E trace records] + the completion mark jh_download_end
 * waits for (timing_done: one event recorded behind the merge, or NULL). */
size_t jh_shard_record_floats(int K, int nu, int mode, int k, int E, int row_floats);
int jh_update_shard(const float* costs, const float* knots_nku, const float* nominal, const float* noise, int ldn, const float* sigma, const float* ctrl_lo_hi, int N,
                    int n_offset, int K, int nu, int mode, float lambda, int k, int tie_high, int E, const float* trace, int row_floats, int colmajor, float* scratch,
                    float* rec_out, void* stream);
int jh_shard_merge(const float* recs, int G, int K, int nu, int mode, float lambda, int k, int tie_high, int E, int row_floats, float* nominal_out, float* sigma_out,
                   float* trace_out, void* stream);
int jh_plan_step_shard(const jh_model* m, void* blk_dev, const void* blk_host, size_t blk_bytes, int o_nominal, int o_sigma, int o_tp, int o_lohi, const float* noise, int ldn,
                       const float* W, int phase, int N, int n_offset, int H, int K, float* costs, float* knots_out, float* trace, int mode, float lambda, int k, int tie_high,
                       int E, int row_floats, int colmajor, float* scratch, float* rec_out, void* const* timing, void* stream);
int jh_plan_merge(const float* recs, int G, int K, int nu, int mode, float lambda, int k, int tie_high, int E, int row_floats, float* out, void* out_host_mark,
                  void* timing_done, void* stream);
/* `timing`: NULL, or three events of jh_event_create recorded on `stream` before the rollout kernel, between it and the update, and behind the update
 * (what bench.py's roofline leg reads: jh_event_elapsed_ms waits for its second event). */
int jh_event_create(void** out);
void jh_event_destroy(void* ev);
int jh_event_record(void* ev, void* stream);
int jh_stream_wait_event(void* stream, void* ev); /* work enqueued on `stream` after this call waits (on the device) for `ev`, recorded on another stream */
int jh_event_elapsed_ms(void* a, void* b, float* ms);
/* Merge G*k records -> global k elites -> mean and clipped population std (ddof 0).  sigma_out may be NULL (PS, k=1). */
int jh_elite_merge(const float* recs, int G, int k, int K, int nu, int tie_high, float sigma_min, float sigma_max, float* nominal_out,
                   float* sigma_out, void* stream);

/* ---- policy half of the Spot policy rollout (mujoco_extensions/system/system_class.cpp:125-238; pybind entry
 * mujoco_extensions/policy_rollout/pybind/policy_rollout.cpp).  One call = System::setObservation + System::policyInference for N rollouts:
 * the 84-d observation from each rollout's state (row stride ld, qpos at 0, qvel at nq; free base at base_qpos / base_qvel, the 19 joints at
 * leg_qpos / leg_qvel), its 25-d command and its previous policy output; the actor 84-512-256-128-12 (Gemm + Elu of spot_locomotion.onnx, weights
 * passed in ONNX layout [out, in]) on exact-f32 MFMA tiles; the mapping to the 19 joint targets.  policy_out (N x 12) is read as the previous output
 * and overwritten with the new one; control is (N x 19); scratch holds jh_policy_scratch_floats(N) floats.  The physics substeps between two policy
 * steps are not part of this call. */
typedef struct jh_policy jh_policy;
int jh_policy_create(const float* const* weights, const float* const* biases, jh_policy** out);
void jh_policy_destroy(jh_policy* p);
size_t jh_policy_scratch_floats(int N);
int jh_policy_step(const jh_policy* p, const float* states, int ld, int nq, int base_qpos, int base_qvel, int leg_qpos, int leg_qvel,
                   const float* command, float* policy_out, float* control, float* scratch, int N, void* stream);

/* ---- physics half of the Spot policy rollout (System::rollout's inner mj_step loop, mujoco_extensions/system/system_class.cpp:300-318): advance
 * N rollouts of a floating-base robot on a ground plane by `substeps` engine steps with the control held.  The model image is what
 * judo_amd/tree_model.py packs (free base + 19 hinges in 5 chains, plane contacts, pyramidal cones, implicitfast; optionally ONE free object: a box, spot_box, or a
 * cylinder, spot_tire; jh_tree_create refuses any other object shape).  state_in / state_out are
 * (N x (nq + nv)) rows [qpos(nq), qvel(nv)] and may alias -- nq / nv = 26 / 25, with the object 33 / 31 (its qpos / qvel after the robot's; jh_tree_dims);
 * ctrl is (N x 19) joint position targets; warmstart (N x nv, may be NULL) is the solver's
 * starting acceleration, read and overwritten with this call's last constraint-consistent acceleration (mjData.qacc_warmstart).  sensors_out (N x nsensordata,
 * may be NULL): mjData.sensordata as mj_step leaves it after the last step, i.e. the site positions / frame axes of that step's forward pass.
 * jh_tree_stats: [contacts dropped over capacity, steps at the iteration cap, Newton iterations, steps]. */
typedef struct jh_tree jh_tree;
int jh_tree_create(const void* blob, size_t nbytes, jh_tree** out);
void jh_tree_destroy(jh_tree* t);
int jh_tree_stats(jh_tree* t, int* out4, int reset);
/* The robot against itself (judo/models/xml/spot_primitive/contact.xml:4-14: every robot geom pair MuJoCo's static filters and the 11 <exclude> body pairs leave, listed
 * in the model image): on by default when the image lists pairs, as MuJoCo collides them; on = 0: the ground contacts only (rounds 1-4). */
int jh_tree_set_self_collision(jh_tree* t, int on);
int jh_tree_dims(const jh_tree* t, int* out4 /* nq, nv, joints (= controls), nsensordata */);
int jh_tree_substeps(const jh_tree* t, const float* state_in, const float* ctrl, float* warmstart, int N, int substeps, float* state_out, float* sensors_out,
                     void* stream);

/* ---- the whole of threaded_rollout (mujoco_extensions/system/system_class.cpp:277-367; pybind entry mujoco_extensions/policy_rollout/pybind/policy_rollout.cpp:65)
 * in the reference's array layouts: x0 is one (nq + nv) state (x0_batched = 0) or (N x (nq + nv)); commands (N x T x 25); states (N x T x (nq + nv)), row [n][i] = the state after
 * command row i's policy step and `substeps` engine steps, sensors (N x T x nsensordata, may be NULL) the sensordata of the same row; policy_out (N x 12) in/out (last_policy_output -> policy_outputs).  warmstart (N x nv, may be NULL)
 * carries mjData.qacc_warmstart from call to call as the reference's per-thread mjData does; reset_warmstart != 0 zeroes it before every control step instead.
 * cutoff_seconds >= 0: the rollout stops issuing command rows once that much DEVICE time has passed since the call started (checked against the control
 * step two back) and the remaining rows repeat the last computed state, as System::rollout does with its wall clock; < 0: no deadline.  *steps_done = rows
 * computed.  scratch holds jh_policy_rollout_scratch_floats(N) floats.  With a deadline the call synchronises with the stream two control steps behind. */
size_t jh_policy_rollout_scratch_floats(int N);
int jh_policy_rollout(const jh_policy* p, jh_tree* t, const float* x0, int x0_batched, const float* commands, float* policy_out, float* warmstart, int reset_warmstart,
                      int N, int T, int substeps, double cutoff_seconds, float* states, float* sensors, float* scratch, int* steps_done, void* stream);
/* threaded_rollout for B problems of n rollouts each in one launch chain (the reference runs one threaded_rollout per controller process,
 * mujoco_extensions/system/system_class.cpp:277-367 under judo/utils/policy_mj_rollout_backend.py:60-125): N = B * n rollouts, problem-major; rollout r starts from problem r / n's
 * state, the B states lying x0_stride_floats apart in DEVICE memory (the x0 parts of a fleet's packed blocks).  commands, policy_out, warmstart, states, sensors, scratch
 * (jh_policy_rollout_scratch_floats(B * n)), reset_warmstart, cutoff_seconds and *steps_done as for jh_policy_rollout with N = B * n; the deadline is one per call.  The
 * start states are copied out to one row per rollout in row T - 1 of `states`, which the last control step overwrites (T = 1: that step reads and writes row 0 in place, as
 * jh_tree_substeps allows).  States, sensors, policy outputs and warm start of
 * problem b are bit for bit those of jh_policy_rollout with N = n from its state: a rollout's result depends neither on its wave-mates nor on the latency mode nor on the
 * policy launch shape its batch size selects.  JH_ERR_INVALID: B < 1, n < 1, x0_stride_floats smaller than a state. */
int jh_policy_rollout_batch(const jh_policy* p, jh_tree* t, int B, const float* x0, size_t x0_stride_floats, const float* commands, float* policy_out, float* warmstart,
                            int reset_warmstart, int n, int T, int substeps, double cutoff_seconds, float* states, float* sensors, float* scratch, int* steps_done, void* stream);

/* ---- a set of P plants for the tree kernel: perturbed copies of one Spot model (masses, inertias, friction, gains: judo_amd/models.py scaled_description), each rollout
 * block of a launch on a plant of the set.  jh_tree_set_create copies the float sections of P jh_trees, 1 <= P <= JH_MAX_ENSEMBLE, into one device allocation, a stride
 * apart that is the float count rounded up to a multiple of 4, and keeps ONE copy of the int section and counters of its own; the trees stay the caller's and may be
 * destroyed.  The members must have member 0's float and int counts, its object kind (none, box, cylinder), an int section identical to member 0's (compared on the
 * host) and its self-collision switch, which becomes the set's; every refusal is JH_ERR_INVALID with jh_last_error naming the member and the section.
 * jh_tree_set_update replaces plant p under the same checks (synchronous: between launches).  jh_tree_set_info: [P, float stride, nq, nv].  jh_tree_set_stats: the
 * four counters of jh_tree_stats, summed over the set's launches. */
typedef struct jh_tree_set jh_tree_set;
int jh_tree_set_create(const jh_tree* const* trees, int P, jh_tree_set** out);
int jh_tree_set_update(jh_tree_set* set, int p, const jh_tree* tree);
int jh_tree_set_info(const jh_tree_set* set, int* out4 /* P, float stride, nq, nv */);
int jh_tree_set_stats(jh_tree_set* set, int* out4, int reset);
void jh_tree_set_destroy(jh_tree_set* set);
/* jh_tree_substeps on G * n block-major rows, block g (rows g * n .. g * n + n - 1) on plant plant_of_block[g] of the set; plant_of_block is a HOST array of G entries in
 * [0, P) that travels in the kernel arguments, G <= JH_MAX_FLEET_PLANT_BLOCKS.  Blocks never share a wave: an odd n leaves one idle row in the last wave of its block.
 * Block g's rows are bit for bit those of jh_tree_substeps with N = n on that plant's own jh_tree.  JH_ERR_INVALID before anything is enqueued, jh_last_error naming the
 * argument: a null pointer, G, n or substeps < 1, G above the limit, a table entry outside [0, P). */
int jh_tree_substeps_plants(const jh_tree_set* set, const int* plant_of_block, int G, int n, const float* state_in, const float* ctrl, float* warmstart, int substeps,
                            float* state_out, float* sensors_out, void* stream);
/* jh_policy_rollout_batch on N = B * G * n rollouts, problem-major then block-major: rollout r starts from problem r / (G * n)'s state and runs on plant
 * plant_of_block[r / n] of the set -- a HOST table of B * G entries in [0, P), problem-major, in the kernel arguments.  The policy step does not depend on the plant and
 * runs on all N rows at once.  commands, policy_out, warmstart, states, sensors, scratch (jh_policy_rollout_scratch_floats(N)), reset_warmstart, cutoff_seconds and
 * *steps_done as documented for jh_policy_rollout_batch with that N; the deadline is one per call.
 * Contract: block (b, g)'s states, sensors, policy outputs and warm start are bit for bit those of jh_policy_rollout with N = n on plant plant_of_block[b * G + g]'s own
 * jh_tree, from problem b's state -- whatever the latency mode and whichever blocks stand beside it.
 * JH_ERR_INVALID before anything is enqueued, jh_last_error naming the argument: a null pointer; B, G, n, T or substeps < 1; B * G > JH_MAX_FLEET_PLANT_BLOCKS; a table
 * entry outside [0, P); x0_stride_floats smaller than a state. */
int jh_policy_rollout_plants(const jh_policy* p, jh_tree_set* set, int B, int G, const int* plant_of_block, const float* x0, size_t x0_stride_floats, const float* commands,
                             float* policy_out, float* warmstart, int reset_warmstart, int n, int T, int substeps, double cutoff_seconds, float* states, float* sensors,
                             float* scratch, int* steps_done, void* stream);

/* ---- jh_rollout_materialize on the plants of a model set: the domain-randomised RolloutBackend.rollout.  G blocks of n rollouts in ONE launch, block g (rows
 * g * n .. g * n + n - 1 of states and sensors) on plant plant_of_block[g] of the set; plant_of_block is a HOST array of G entries in [0, M) that travels in the kernel
 * arguments, G <= JH_MAX_FLEET_PLANT_BLOCKS, M <= JH_MAX_ENSEMBLE.  x0 is one state (nq+nv) or, when x0_batched, one per row (G * n, nq+nv).  controls are (G * n, H, nu),
 * block g's own n rows, or, when controls_shared, (n, H, nu): rows [0, n) for every block -- an ensemble rolls the same candidates out on every plant without copying
 * them M times.  states (G * n, H, nq+nv) and sensors (G * n, H, nsensordata) as for jh_rollout_materialize; one of the two may be NULL.  Blocks never share a wave or a
 * workgroup: a ragged last workgroup, or an idle row of a block's last wave, ends at its own block's last rollout.  The int section (topology, pair lists) is the set's
 * one copy, as for the plan steps on a set.  Families: cartpole, cylinder_push and the leap family (kernel generation 3: 48 contacts, 64 contacts, cylinders; the hand's
 * own contacts on or off).
 * Contract: rows [g * n, (g + 1) * n) of states and sensors are bit for bit what jh_rollout_materialize writes on plant plant_of_block[g]'s own jh_model for those n rows
 * (its x0 and controls), whatever the latency mode the launch's G * n rollouts select and whichever blocks stand beside it.
 * JH_ERR_INVALID before anything is enqueued, jh_last_error naming the argument: a null pointer (set, plant_of_block, x0, controls); states and sensors both NULL; G
 * outside 1..JH_MAX_FLEET_PLANT_BLOCKS; n or H < 1; a table entry outside [0, M) (named with its block); G * n beyond the 2^31 - 1 rollouts of one launch.
 * JH_ERR_UNSUPPORTED: a set of fr3_pick models (jh_fr3_model_set_create) -- behind this entry the arm kernel has no materialise launch on plants;
 * jh_fr3_rollout_materialize_plants below is that launch --, or a member 0 switched to another kernel generation. */
int jh_rollout_materialize_plants(const jh_model_set* set, const int* plant_of_block, int G, int n, const float* x0, int x0_batched, const float* controls, int controls_shared,
                                  int H, float* states, float* sensors, void* stream);

/* ---- jh_rollout_materialize_plants for a set of fr3_pick models (jh_fr3_model_set_create): the cooperative arm kernel's materialise launch on plants, behind an entry of
 * its own as every fr3 form is.  The arguments, their shapes and their limits are those of jh_rollout_materialize_plants; both builds of the arm kernel (the shipped
 * pairs, the arm's own pairs) serve it, chosen by the set's member 0 as for jh_rollout_materialize.  Grid (waves of a block, G): blocks never share a wave, and an idle
 * row of a block's last wave ends at its own block's last rollout.  The int section is member 0's own, which an fr3 set's members share word for word.  The launch has
 * no phase: materialise mode evaluates every distance sensor and computes no cost (jh_task_reward takes the phase).  The counters are member 0's (jh_model_stats).
 * Contract: rows [g * n, (g + 1) * n) of states and sensors are bit for bit what jh_rollout_materialize writes on plant plant_of_block[g]'s own jh_model for those n rows
 * (its x0 and controls), whatever the latency mode the launch's G * n rollouts select and whichever blocks stand beside it.
 * JH_ERR_INVALID before anything is enqueued, jh_last_error naming the argument: as for jh_rollout_materialize_plants.
 * JH_ERR_UNSUPPORTED: a set that is not of fr3_pick models (jh_rollout_materialize_plants rolls it out). */
int jh_fr3_rollout_materialize_plants(const jh_model_set* set, const int* plant_of_block, int G, int n, const float* x0, int x0_batched, const float* controls, int controls_shared,
                                      int H, float* states, float* sensors, void* stream);

/* ---- jh_plant_residuals: the scoring half of plant identification.  W recorded windows of H steps were rolled out on all M plants of a set (one materialise launch on
 * plants: M blocks of W rows, the windows' x0 tiled M times, their controls shared), and err[m * ld + w] is the weighted squared prediction error of plant m on window w.
 * pred is what that launch wrote, (M * W, H, nx) with block m = rows [m * W, (m + 1) * W); obs (W, H, nx) the observed states; weight (nx) per-coordinate weights,
 * 1 / sigma^2.  quat_adr is a HOST array of nquat offsets into a state row, each naming four consecutive coordinates of a unit quaternion inside [0, nq); it travels in
 * the kernel arguments, nquat <= JH_MAX_ID_QUATS.  H <= JH_MAX_ID_HORIZON, the wave width.  What lies between W and ld in a row of err is not written.
 * The arithmetic is fixed, all of it in fp32 with every product and sum rounded on its own (no fused multiply-add), so that a host restatement matches bit for bit
 * (judo_amd/identify.py plant_residuals_host):
 *   per step and quaternion   dot = ((p0 * o0 + p1 * o1) + p2 * o2) + p3 * o3; if dot < 0 the prediction is compared against -o: a pose and its antipodal quaternion
 *                             have error exactly 0;
 *   per coordinate d          e = p - o', t_d = (weight[d] * e) * e;
 *   per step h                s_h = ((t_0 + t_1) + t_2) + ..., d ascending;
 *   per window                v[0..63] = s_0 .. s_{H-1}, then +0.0; six halvings v[i] = v[i] + v[i + k], k = 32, 16, 8, 4, 2, 1; err = v[0] -- the order of a wave-wide
 *                             butterfly with one wave per (m, w) pair and lane h holding step h.  The padding is exact: every term is non-negative.
 * Non-finite inputs are outside the contract: NaN in gives NaN out (judo_amd.identify.PlantEstimator counts such an error as +inf).
 * JH_ERR_INVALID before anything is enqueued, jh_last_error naming the argument: a null pred, obs, weight or err; M outside 1..JH_MAX_ENSEMBLE; W < 1; H outside
 * 1..JH_MAX_ID_HORIZON; nx < 1; nq outside 0..nx; ld < W; nquat outside 0..JH_MAX_ID_QUATS; nquat > 0 with a null quat_adr; an offset that is negative, reaches past nq
 * with its four coordinates, or overlaps another offset; M * W beyond the workgroups of one launch. */
int jh_plant_residuals(const float* pred /* DEVICE, (M * W, H, nx) */, const float* obs /* DEVICE, (W, H, nx) */, const float* weight /* DEVICE, nx */,
                       const int* quat_adr /* HOST, nquat offsets, or NULL with nquat = 0 */, int nquat, int M, int W, int H, int nx, int nq, float* err /* DEVICE, M x ld */,
                       int ld, void* stream);

/* ---- jh_plant_residuals_reports: jh_plant_residuals for a robot's reports.  An entry of obs or obs_sens that is NaN was NOT REPORTED: it is no evidence for or against
 * any plant.  One rule covers reports slower than the model's step (whole step rows are NaN), partial reports (the velocity columns are NaN) and dropped readings.
 * Sensor readings can be evidence beside the states, and the predictions may lie plant-major or window-major.
 * Layout: the prediction of plant m on window w is window-row m * plant_stride + w * window_stride of pred, a window-row being (H, nx), contiguous; the same window-row
 * index addresses pred_sens, whose rows are (H, ns) -- states and sensors come out of one launch in the same rollout order.  The plants launch of a model set is
 * plant-major (plant_stride = W, window_stride = 1); jh_policy_rollout_plants with a problem per window is window-major (plant_stride = 1, window_stride = M).  Both
 * strides are at least 1.  obs is (W, H, nx), obs_sens (W, H, ns); weight (nx) and weight_sens (ns) are 1 / sigma^2.  ns = 0 with three null sensor pointers: no sensor
 * evidence.  quat_adr, nquat, nq, H, ld: as for jh_plant_residuals.
 * The arithmetic is fixed, all of it in fp32 with every product and sum rounded on its own (no fused multiply-add); judo_amd/reports.py plant_residuals_reports_host
 * restates it bit for bit:
 *   per step and quaternion   dot = ((p0 * o0 + p1 * o1) + p2 * o2) + p3 * o3 as in jh_plant_residuals; a NaN among the four observed coordinates makes dot NaN, hence
 *                             no flip;
 *   per state coordinate d    if obs[d] is NaN -- on the bits: (bits & 0x7fffffff) > 0x7f800000 -- t_d = +0.0, and neither pred[d] nor weight[d] enters; otherwise
 *                             e = p - o', t_d = (weight[d] * e) * e;
 *   per step h                s_h = t_0, then s_h = s_h + t_d, d ascending; the ns sensor coordinates continue the same sum in ascending order under the same NaN rule
 *                             with weight_sens (they have no quaternions);
 *   per window                the 64-slot halving of jh_plant_residuals.
 * With no NaN in obs, ns = 0 and plant-major strides the result is bit for bit that of jh_plant_residuals: a skipped term adds +0.0 to a non-negative sum, which is
 * exact.  A window with nothing reported has error exactly +0.0 for every plant.  A NaN prediction under a reported entry gives NaN out (the estimators count it as
 * +inf); under an unreported one it is not read into the sum.  Observed infinities are outside the contract.
 * JH_ERR_INVALID before anything is enqueued, jh_last_error naming the argument: everything jh_plant_residuals refuses; ns < 0; ns > 0 with a null pred_sens, obs_sens
 * or weight_sens; ns = 0 with one of them not null; a stride of 0. */
int jh_plant_residuals_reports(const float* pred /* DEVICE, window-rows of (H, nx) */, const float* obs /* DEVICE, (W, H, nx) */, const float* weight /* DEVICE, nx */,
                               const int* quat_adr /* HOST, nquat offsets, or NULL with nquat = 0 */, int nquat, const float* pred_sens /* DEVICE, window-rows of (H, ns), or NULL */,
                               const float* obs_sens /* DEVICE, (W, H, ns), or NULL */, const float* weight_sens /* DEVICE, ns, or NULL */, int ns, size_t plant_stride,
                               size_t window_stride, int M, int W, int H, int nx, int nq, float* err /* DEVICE, M x ld */, int ld, void* stream);

/* ---- The plant side of the closed loop (judo/app/dora/simulation.py:52-82, judo/simulation/mj_simulation.py:33-46, for B plants at once): B device-resident plants
 * advance S physics steps on the splines their controllers planned.  judo_amd/simulation.py restates the two kernels' arithmetic (plant_controls_host,
 * plant_reports_host) and holds the plants (PlantFleet).  All arithmetic in fp32, every product and sum rounded on its own (no fused multiply-add).
 *
 * jh_plant_controls: B splines at their plants' own clocks.  controls[b, step0 + s, u] = sum_k W[b, s, k] * knots[b, k, u] for s < S: acc = W[b,s,0] * knots[b,0,u],
 * then acc = acc + W[b,s,k] * knots[b,k,u], k ascending; then, where ctrl_lo_hi (nu lower bounds, then nu upper bounds) is given, acc < lo -> lo and acc > hi -> hi in
 * the order of the values' bits (-0.0 below +0.0; a NaN passes through).  W is (B, S, K), plant b's rows built on the host by spline_weights for its knot times and its
 * clock; knots are (K, nu) per plant, knot_stride floats from one plant's to the next; controls is (B, ld_steps, nu), so a call fills steps step0 .. step0 + S - 1 of a
 * longer segment and writes no other word.  Grid (workgroups over S * nu, B).
 * JH_ERR_INVALID before anything is enqueued, jh_last_error naming the argument: a null W, knots or controls; B outside 1..JH_MAX_FLEET_PLANT_BLOCKS; S, K or nu < 1;
 * K * nu > JH_MAX_KNOT_DIM; B > 1 with knot_stride < K * nu; step0 < 0; ld_steps < step0 + S. */
int jh_plant_controls(const float* W /* DEVICE, (B, S, K) */, const float* knots /* DEVICE */, size_t knot_stride, const float* ctrl_lo_hi /* DEVICE, 2 * nu, or NULL */, int B,
                      int S, int K, int nu, int step0, int ld_steps, float* controls /* DEVICE, (B, ld_steps, nu) */, void* stream);

/* jh_plant_reports: what a robot reports of a segment, and the carry.  states is (B, S, nx) and sensors (B, S, ns) as a materialise launch wrote them.
 *   reports[b, s, j] = states[b, s, j] + sigma[j] * noise[b, s, j] (the product, then the sum) where step s of plant b and column j are reported; just states[b, s, j]
 *   where sigma or noise is NULL; NaN (0x7fc00000) where the step or the column is not reported.  noise is (B, S, nx), what jh_noise_normal(seed, draw, B * S, 0, nx,
 *   noise, nx) draws.  Step s of plant b is reported when (count[b] + s + 1) % every == 0, count[b] being the steps plant b has taken before the segment: a stride that
 *   does not divide S carries across segments.  Column j is reported when column_mask[j] != 0 (nx bytes on the device), or always with a NULL mask.
 *   reports_sens likewise from sensors with noise_sens (B, S, ns), sigma_sens and column_mask_sens (ns); NULL: no sensor reports.
 *   x[b, :] = states[b, S - 1, :]: the exact state, never the noisy one.
 * With sigma NULL, every == 1 and no mask the reports are the states bit for bit.  With reports and reports_sens NULL the launch only carries.
 * JH_ERR_INVALID before anything is enqueued: a null states, x or count; B outside 1..JH_MAX_FLEET_PLANT_BLOCKS; S or nx < 1; ns < 0; every < 1; a negative count,
 * named with its plant; reports_sens with ns = 0 or a null sensors. */
int jh_plant_reports(const float* states, const float* sensors /* or NULL */, int B, int S, int nx, int ns, const int* count /* HOST, B */, int every, const float* noise,
                     const float* sigma, const unsigned char* column_mask, float* reports /* DEVICE, (B, S, nx), or NULL */, const float* noise_sens, const float* sigma_sens,
                     const unsigned char* column_mask_sens, float* reports_sens /* DEVICE, (B, S, ns), or NULL */, float* x /* DEVICE, (B, nx) */, void* stream);

/* jh_plants_advance: the whole chain in one call, three launches on `stream`:
 *   1. k_plant_controls for steps step0 .. S - 1 of controls (B, S, nu) from W (B, S - step0, K) -- with step0 > 0 the caller has filled steps 0 .. step0 - 1 with a
 *      jh_plant_controls call of its own: a plan that takes effect step0 steps after the state it was planned from;
 *   2. the materialise launch on plants -- the launcher behind jh_rollout_materialize_plants, or behind jh_fr3_rollout_materialize_plants for an fr3_pick set --
 *      with G = B blocks of n = 1 row, block b on plant truth[b], x0 batched from x (B, nq + nv), a row of controls per plant, H = S;
 *   3. k_plant_reports, which also carries x.
 * Contract: rows b of states (B, S, nq + nv) and sensors (B, S, nsensordata; may be NULL) are bit for bit what jh_rollout_materialize writes on plant truth[b]'s own
 * jh_model from x[b] with those S controls.  x stays on the device between calls.
 * The leap and fr3 kernels start their contact solver cold at the top of a launch: a plant carries the solver's warm start within a segment and not across segments
 * (a MuJoCo plant carries qacc_warmstart from step to step).  DESIGN.md section 4.21.
 * JH_ERR_INVALID before the first enqueue, jh_last_error naming the argument: everything the two entries above refuse; a null set or truth; step0 outside [0, S); a set
 * of more than JH_MAX_ENSEMBLE members; a truth entry outside [0, M), named with its plant.  JH_ERR_UNSUPPORTED: a set whose member 0 runs another kernel generation
 * than 3.  The set is a jh_model_set: a Spot tree set (jh_tree_set) is another type, its plant carries policy state and a solver warm start, and
 * judo_amd.simulation.PlantFleet refuses it by name. */
int jh_plants_advance(const jh_model_set* set, const int* truth /* HOST, B */, int B, float* x /* DEVICE, (B, nq + nv) */, const float* W /* DEVICE, (B, S - step0, K) */,
                      const float* knots /* DEVICE */, size_t knot_stride, int K, const float* ctrl_lo_hi /* DEVICE, 2 * nu, or NULL */, int step0, int S,
                      float* controls /* DEVICE, (B, S, nu) */, float* states /* DEVICE, (B, S, nq + nv) */, float* sensors /* DEVICE, (B, S, nsensordata), or NULL */,
                      const int* count /* HOST, B */, int every, const float* noise, const float* sigma, const unsigned char* column_mask, float* reports, const float* noise_sens,
                      const float* sigma_sens, const unsigned char* column_mask_sens, float* reports_sens, void* stream);

#ifdef __cplusplus
}
#endif
#endif
