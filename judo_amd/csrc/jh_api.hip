// jh_api.hip -- C-ABI entry points of libjudo_amd.so (argument checks, model handles, dispatch).
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>

#include "jh_internal.h"
#include "jh_update_dev.h"

static thread_local char g_err[512] = "";

void jh_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

extern "C" const char* jh_last_error(void) { return g_err; }
extern "C" int jh_version(void) { return 100; }

using jh_eng::HI_PT;

static bool blob_sections(const void* blob, size_t nbytes, std::vector<float>& F, std::vector<int>& I) {
  jh_blob_header h;
  if (!blob || nbytes < sizeof(h)) return false;
  memcpy(&h, blob, sizeof(h));
  if (h.magic != JH_BLOB_MAGIC || nbytes != sizeof(h) + 4 * ((size_t)h.nfloat + h.nint)) return false;
  const char* q = (const char*)blob + sizeof(h);
  F.assign((const float*)q, (const float*)q + h.nfloat);
  I.assign((const int*)(q + 4 * (size_t)h.nfloat), (const int*)(q + 4 * (size_t)h.nfloat) + h.nint);
  return true;
}

// The model-set rule on two packed images, without a device: 1 if a set of the two keeps the pair tables of `blob0`, 0 if it runs without them.
extern "C" int jh_pair_tables_shared(const void* blob0, size_t nbytes0, const void* blob, size_t nbytes) {
  std::vector<float> F0, F; std::vector<int> I0, I;
  JH_REQUIRE(blob_sections(blob0, nbytes0, F0, I0) && blob_sections(blob, nbytes, F, I), "pair_tables_shared: not a model blob");
  jh_eng::HostImage a, b;
  a.bind(F0.data(), I0.data(), F0.size(), I0.size()); b.bind(F.data(), I.data(), F.size(), I.size());
  return jh_eng::pair_tables_shared(a, b) ? 1 : 0;
}

extern "C" int jh_model_create(const void* blob, size_t nbytes, int device, jh_model** out) {
  JH_REQUIRE(blob && out, "model_create: null pointer");
  if (nbytes < sizeof(jh_blob_header)) { jh_set_error("model_create: blob too small (%zu bytes)", nbytes); return JH_ERR_BLOB; }
  jh_blob_header h;
  memcpy(&h, blob, sizeof(h));
  if (h.magic != JH_BLOB_MAGIC || h.version != JH_BLOB_VERSION) { jh_set_error("model_create: bad magic/version (%08x, %u)", h.magic, h.version); return JH_ERR_BLOB; }
  size_t need = sizeof(h) + 4 * ((size_t)h.nfloat + h.nint);
  if (nbytes != need) { jh_set_error("model_create: blob size %zu != expected %zu", nbytes, need); return JH_ERR_BLOB; }
  if (h.kind > JH_TASK_FR3_PICK) { jh_set_error("model_create: unknown task kind %u", h.kind); return JH_ERR_BLOB; }
  if (h.kind == JH_TASK_CARTPOLE && h.nfloat < CP_NPARAM) { jh_set_error("model_create: cartpole blob has %u floats, need %d", h.nfloat, CP_NPARAM); return JH_ERR_BLOB; }
  if (h.kind == JH_TASK_CYLINDER_PUSH && h.nfloat < CY_NPARAM) { jh_set_error("model_create: cylinder blob has %u floats, need %d", h.nfloat, CY_NPARAM); return JH_ERR_BLOB; }
  if (h.ntaskparam > JH_MAX_TASK_PARAMS) { jh_set_error("model_create: too many task params"); return JH_ERR_BLOB; }
  const char* p = (const char*)blob + sizeof(h);
  std::vector<float> F((const float*)p, (const float*)p + h.nfloat);  // (copies: the blob need not be aligned; the model keeps them)
  std::vector<int> I((const int*)(p + 4 * (size_t)h.nfloat), (const int*)(p + 4 * (size_t)h.nfloat) + h.nint);
  // The articulated kinds: the view of the image and whether it fits, once, for the readers here and for every launch's acceptance test.  An image that does not fit is
  // still a model (not an engine image: the launchers refuse it).
  jh_eng::HostImage image;
  int cylinders = 0, arm_pairs = 0;
  if (h.kind == JH_TASK_LEAP_CUBE || h.kind == JH_TASK_FR3_PICK) {
    image.bind(F.data(), I.data(), F.size(), I.size());
    const jh_eng::EngineModel& v = image.v;
    image.fits = image.fits && v.NQ == (int)h.nq && v.NV == (int)h.nv && v.NU == (int)h.nu && v.NS == (int)h.ns;  // (the kernels size their loops by the image's counts, the launchers their buffers by the blob header's)
    cylinders = jh_eng::image_cylinders(image);
    if (cylinders < 0) return JH_ERR_BLOB;
    if (h.kind == JH_TASK_LEAP_CUBE && jh_eng::image_pair_tables(image) < 0) return JH_ERR_BLOB;
    if (cylinders > 0 && h.kind != JH_TASK_LEAP_CUBE) { jh_set_error("model_create: %d cylinder geoms, and only the leap kernel has a cylinder build", cylinders); return JH_ERR_BLOB; }
    if (h.kind == JH_TASK_FR3_PICK) {
      arm_pairs = jh_eng::image_arm_pairs(image);
      if (arm_pairs < 0) return JH_ERR_BLOB;
    }
  }
  JH_HIP(hipSetDevice(device));
  jh_model* m = new jh_model();
  m->device = device; m->kind = (int)h.kind; m->nq = h.nq; m->nv = h.nv; m->nu = h.nu; m->ns = h.ns; m->ntaskparam = h.ntaskparam;
  m->nf = h.nfloat; m->ni = h.nint; m->d_f = nullptr; m->d_i = nullptr; m->d_stats = nullptr; m->kernel_gen = (h.kind == JH_TASK_LEAP_CUBE || h.kind == JH_TASK_FR3_PICK) ? 3 : 2; m->self_collision = 1; m->contact_capacity = cylinders > 0 ? 64 : 48; m->cylinders = cylinders; m->arm_pairs = arm_pairs;
  { const char* e = getenv("JUDO_AMD_ROLLOUT_SCHEDULE"); m->rollout_schedule = (e && (e[0] == '1' || e[0] == '2')) ? e[0] - '0' : 0; }  // (the environment sets the default; jh_model_set_rollout_schedule changes it per model)
  { const char* e = getenv("JUDO_AMD_ROLLOUT_SLICES"); const int v = e ? atoi(e) : 0; m->rollout_slices = (v >= 1 && v <= 64) ? v : 0; }  // (likewise; jh_model_set_rollout_slices)
  if (const char* e = getenv("JUDO_AMD_ROLLOUT_SLICE_BOUNDS")) {  // (likewise, and in front of the number above where both are set; "24,40,52,60"; jh_model_set_rollout_slice_bounds; a list it would refuse is ignored)
    int b[JH_MAX_SLICE_BOUNDS + 1], n = 0; bool ok = true;
    for (const char* p = e; *p && ok;) { char* q; const long v = strtol(p, &q, 10); ok = q != p && n <= JH_MAX_SLICE_BOUNDS - 1 && v > (n ? b[n - 1] : 0) && v < (1l << 30) && (*q == ',' || *q == 0); if (ok) { b[n++] = (int)v; p = *q ? q + 1 : q; } }
    if (ok && n > 0) { for (int i = 0; i < n; i++) m->rollout_bounds[i] = b[i]; m->rollout_nbounds = n; m->rollout_slices = 0; }
  }
  { const char* e = getenv("JUDO_AMD_PLAN_STEP_LAUNCHES"); m->plan_step_launches = (e && e[0] == '2') ? 2 : 0; }  // (the environment sets the default; jh_model_set_plan_step_launches changes it per model)
  m->h_f = std::move(F); m->h_i = std::move(I); m->image = image;  // (a moved vector keeps its storage: the view's pointers hold)
  {  // the cooperative kernels take a per-launch scratch block from the device's stream-ordered pool (contacts above the LDS pool): let the pool keep what it is
     // handed back instead of returning it to the driver at every synchronisation (the default release threshold is 0: 0.2 ms per launch)
    hipMemPool_t pool = nullptr; int dev = 0;
    if (hipGetDevice(&dev) == hipSuccess && hipDeviceGetDefaultMemPool(&pool, dev) == hipSuccess && pool) {
      unsigned long long keep = ~0ull;
      (void)hipMemPoolSetAttribute(pool, hipMemPoolAttrReleaseThreshold, &keep);
    }
  }
  hipError_t e = hipMalloc(&m->d_f, 4 * (m->nf ? m->nf : 1));
  if (e == hipSuccess) e = hipMalloc(&m->d_i, 4 * (m->ni ? m->ni : 1));
  if (e == hipSuccess) e = hipMalloc(&m->d_stats, JH_NSTATS * sizeof(int));
  if (e == hipSuccess) e = hipMemset(m->d_stats, 0, JH_NSTATS * sizeof(int));
  if (e == hipSuccess && m->nf) e = hipMemcpy(m->d_f, m->h_f.data(), 4 * m->nf, hipMemcpyHostToDevice);
  if (e == hipSuccess && m->ni) e = hipMemcpy(m->d_i, m->h_i.data(), 4 * m->ni, hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    jh_set_error("model_create: device upload failed: %s", hipGetErrorString(e));
    if (m->d_f) (void)hipFree(m->d_f);
    if (m->d_i) (void)hipFree(m->d_i);
    if (m->d_stats) (void)hipFree(m->d_stats);
    delete m;
    return JH_ERR_HIP;
  }
  *out = m;
  return JH_OK;
}

extern "C" void jh_model_destroy(jh_model* m) {
  if (!m) return;
  if (m->d_f) (void)hipFree(m->d_f);
  if (m->d_i) (void)hipFree(m->d_i);
  if (m->d_stats) (void)hipFree(m->d_stats);
  delete m;
}

extern "C" int jh_model_dims(const jh_model* m, int* dims) {
  JH_REQUIRE(m && dims, "model_dims: null pointer");
  dims[0] = m->nq; dims[1] = m->nv; dims[2] = m->nu; dims[3] = m->ns; dims[4] = m->kind; dims[5] = m->ntaskparam;
  return JH_OK;
}

extern "C" int jh_model_stats(jh_model* m, int* out, int reset) {
  JH_REQUIRE(m && out, "model_stats: null pointer");
  JH_HIP(hipMemcpy(out, m->d_stats + JH_STAT_DROPS, 4 * sizeof(int), hipMemcpyDeviceToHost));  // (... JH_STAT_STEPS)
  JH_HIP(hipMemcpy(out + 4, m->d_stats + JH_STAT_WAVE_ITERS, 2 * sizeof(int), hipMemcpyDeviceToHost));  // (and JH_STAT_WAVE_STEPS)
  out[6] = reset ? __atomic_exchange_n(&m->ovf_fallbacks, 0, __ATOMIC_RELAXED) : __atomic_load_n(&m->ovf_fallbacks, __ATOMIC_RELAXED);
  out[7] = reset ? __atomic_exchange_n(&m->one_launch_steps, 0, __ATOMIC_RELAXED) : __atomic_load_n(&m->one_launch_steps, __ATOMIC_RELAXED);
  if (reset) JH_HIP(hipMemset(m->d_stats, 0, JH_NSTATS * sizeof(int)));
  return JH_OK;
}

extern "C" int jh_model_hist(jh_model* m, int* out /* 24 ints: Newton-iteration histogram (profile builds only) */) {
  JH_REQUIRE(m && out, "model_hist: null pointer");
  JH_HIP(hipMemcpy(out, m->d_stats + 24, 40 * sizeof(int), hipMemcpyDeviceToHost));
  return JH_OK;
}

extern "C" int jh_model_counters(jh_model* m, int* out, int first, int count) {  // diagnostic builds (JH_V5_CENSUS ...): a range of the raw counter block
  JH_REQUIRE(m && out && first >= 0 && count >= 0 && first + count <= JH_NSTATS, "model_counters: bad range");
  JH_HIP(hipMemcpy(out, m->d_stats + first, count * sizeof(int), hipMemcpyDeviceToHost));
  return JH_OK;
}

static jh_xcheck_launchers g_xcheck = {nullptr, nullptr, nullptr};

extern "C" int jh_register_xcheck(const jh_xcheck_launchers* launchers) {
  JH_REQUIRE(launchers && launchers->rollout_cost && launchers->rollout_materialize && launchers->max_knots, "register_xcheck: incomplete launcher table");
  g_xcheck = *launchers;
  return JH_OK;
}

// The build that runs a model: the one place that chooses among the rows of jh_internal.h.  The closed-form models: their one row, whatever generation is set on them.
// The leap family: the cylinder build for an image with cylinders, else the 64-contact build where jh_model_set_contact_capacity asked for it, else the 48-contact one;
// fr3: the self-collision build for an image with arm pairs, else the default.  Null: a cross-check generation of an articulated model (g_xcheck), and nothing else.
static const jh_engine_build* engine_build(const jh_model* m) {
  if (m->kind == JH_TASK_CARTPOLE || m->kind == JH_TASK_CYLINDER_PUSH) return &jh_simple_build;
  if (m->kernel_gen != 3) return nullptr;
  if (m->kind == JH_TASK_LEAP_CUBE) return m->cylinders > 0 ? &jh_engine5_build_cyl : m->contact_capacity > 48 ? &jh_engine5_build_cap64 : &jh_engine5_build;
  if (m->kind == JH_TASK_FR3_PICK) return m->arm_pairs > 0 ? &jh_engine6_build_self : &jh_engine6_build;
  return nullptr;
}

// A model whose row serves it under every kernel generation: setting one has no effect on it and needs no cross-check library.
static bool every_generation(const jh_model* m) { return engine_build(m) == &jh_simple_build; }

extern "C" int jh_model_set_kernel(jh_model* m, int generation) {
  JH_REQUIRE(m && generation >= 1 && generation <= 3, "model_set_kernel: generation must be 1, 2 or 3");
  if (generation != 3 && !every_generation(m) && !g_xcheck.rollout_cost) {
    jh_set_error("model_set_kernel: generations 1 and 2 are cross-check kernels of the test build (libjudo_amd_xcheck.so), not part of this library");
    return JH_ERR_UNSUPPORTED;
  }
  if (generation != 3 && m->cylinders > 0) {
    jh_set_error("model_set_kernel: the image holds %d cylinder geoms; only generation 3 (the cylinder build of the leap kernel) collides them", m->cylinders);
    return JH_ERR_UNSUPPORTED;
  }
  if (generation != 3 && m->arm_pairs > 0) {
    jh_set_error("model_set_kernel: the image holds %d pairs between arm bodies; only generation 3 (the self-collision build of the fr3 kernel) collides them", m->arm_pairs);
    return JH_ERR_UNSUPPORTED;
  }
  m->kernel_gen = generation;
  return JH_OK;
}

// trace sensors the model's fused kernel can write per rollout and step: its row's answer, and none for a cross-check generation
static jh_trace_layout trace_layout(const jh_model* m) {
  const jh_engine_build* eb = engine_build(m);
  return eb && eb->trace_layout ? eb->trace_layout(m) : jh_trace_layout{};
}

extern "C" int jh_model_trace_layout(const jh_model* m, int* out) {
  JH_REQUIRE(m && out, "model_trace_layout: null pointer");
  const jh_trace_layout t = trace_layout(m);
  out[0] = t.adr; out[1] = t.floats; out[2] = t.colmajor;
  return JH_OK;
}

extern "C" int jh_model_set_contact_capacity(jh_model* m, int contacts) {
  JH_REQUIRE(m != nullptr, "model_set_contact_capacity: null pointer");
  JH_REQUIRE(m->kind == JH_TASK_LEAP_CUBE && (contacts == 48 || contacts == 64), "model_set_contact_capacity: the leap_cube kernel is built for 48 and for 64 contacts per rollout (got %d)", contacts);
  JH_REQUIRE(m->cylinders == 0 || contacts == 64, "model_set_contact_capacity: the cylinder build of the leap kernel holds 64 contacts per rollout (got %d)", contacts);
  m->contact_capacity = contacts;
  return JH_OK;
}

extern "C" int jh_model_build(const jh_model* m, int* out) {
  JH_REQUIRE(m && out, "model_build: null pointer");
  out[0] = m->kernel_gen;
  const jh_engine_build* eb = engine_build(m);
  out[1] = eb && m->kind == JH_TASK_LEAP_CUBE ? eb->contact_capacity : 0;
  out[2] = eb == &jh_engine5_build_cyl ? 1 : 0;
  out[3] = m->cylinders;
  return JH_OK;
}

extern "C" int jh_model_fr3_build(const jh_model* m, int* out) {
  JH_REQUIRE(m && out, "model_fr3_build: null pointer");
  const bool fr3 = m->kind == JH_TASK_FR3_PICK;
  out[0] = engine_build(m) == &jh_engine6_build_self ? 1 : 0;
  out[1] = fr3 ? m->arm_pairs : 0;
  out[2] = fr3 && jh_engine6_build.accepts(m) ? 1 : 0;
  out[3] = fr3 && jh_engine6_build_self.accepts(m) ? 1 : 0;
  return JH_OK;
}

extern "C" int jh_model_set_self_collision(jh_model* m, int on) {
  JH_REQUIRE(m != nullptr, "model_set_self_collision: null pointer");
  m->self_collision = on ? 1 : 0;
  return JH_OK;
}

int jh_latency_shift(int N, int rpw) {
  static int cus = 0;
  if (cus == 0) { int dev = 0, v = 0; cus = (hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && v > 0) ? v : 256; }
  int most = 0; while ((2 << most) <= rpw) most++;
  const char* e = getenv("JUDO_AMD_LATENCY_SHIFT");  // diagnostic override: 0 = every row its own rollout, always
  if (e && e[0] >= '0' && e[0] <= '2') return (e[0] - '0') < most ? (e[0] - '0') : most;
  const long alone = (long)cus * 4;  // waves that each have a SIMD to themselves: a second wave on a SIMD takes from the first what the copies would gain
  for (int sh = most; sh > 0; sh--) if (((long)N << sh) <= alone * rpw) return sh;
  return 0;
}

static int max_fused_knots(const jh_model* m, int H) {
  const int k = JH_MAX_KNOT_DIM / (m->nu > 0 ? m->nu : 1);
  const jh_engine_build* eb = engine_build(m);
  int own = k;  // the build's own bound, where it has one
  if (eb && eb->max_fused_knots) own = eb->max_fused_knots(m, H);
  // the cross-check generations: the cooperative one keeps 8 knots per actuator in registers; the one-lane kernel stages W (H x K) and 64 lanes' knots in LDS, and the
  // launcher's 64 KiB budget bounds K as well
  if (!eb) own = m->kernel_gen >= 2 ? 8 : (g_xcheck.max_knots ? g_xcheck.max_knots(m, H) : 0);
  return k < own ? k : own;
}

extern "C" int jh_model_limits(const jh_model* m, int* out) {
  JH_REQUIRE(m && out, "model_limits: null pointer");
  out[0] = max_fused_knots(m, 1);  // upper bound over all horizons; jh_model_max_fused_knots(m, H) is the figure for a given H
  out[1] = JH_MAX_KNOT_DIM;
  out[2] = JH_MAX_ELITES;
  const jh_engine_build* eb = engine_build(m);
  out[3] = eb ? eb->contact_capacity : 32;  // (generation 3: leap 48, all in LDS, or 64 with 16 in a row of global memory: jh_model_set_contact_capacity; fr3 32 in LDS + 64 in such a row, next to its 96 pad-against-pad slots; the closed-form models: 0; the cross-check generations: 32)
  return JH_OK;
}

extern "C" int jh_model_max_fused_knots(const jh_model* m, int H) {
  JH_REQUIRE(m != nullptr && H >= 1, "model_max_fused_knots: null model or H < 1");
  return max_fused_knots(m, H);
}

extern "C" int jh_model_one_launch_max_knots(const jh_model* m, int H) {
  JH_REQUIRE(m != nullptr && H >= 1, "model_one_launch_max_knots: null model or H < 1");
  const jh_engine_build* eb = engine_build(m);
  const int k = JH_MAX_KNOT_DIM / (m->nu > 0 ? m->nu : 1), lds_k = eb && eb->plan_step ? eb->one_launch_max_knots(m, H) : 0;
  return k < lds_k ? k : lds_k;
}

extern "C" int jh_model_set_plan_step_launches(jh_model* m, int launches) {
  JH_REQUIRE(m != nullptr && launches >= 0 && launches <= 2, "model_set_plan_step_launches: launches must be 0 (automatic), 1 or 2");
  const jh_engine_build* eb = engine_build(m);
  JH_REQUIRE(launches != 1 || (eb && eb->plan_step), "model_set_plan_step_launches: only the closed-form models have a one-launch plan step");
  m->plan_step_launches = launches;
  return JH_OK;
}

extern "C" int jh_model_set_rollout_schedule(jh_model* m, int mode) {
  JH_REQUIRE(m != nullptr && mode >= 0 && mode <= 2, "model_set_rollout_schedule: mode must be 0 (automatic), 1 (static grid) or 2 (persistent waves wherever the kernel has them)");
  m->rollout_schedule = mode;
  return JH_OK;
}

extern "C" int jh_model_set_rollout_slices(jh_model* m, int slices, int max_workgroups, int flags) {
  JH_REQUIRE(m != nullptr && slices >= 0 && slices <= 64, "model_set_rollout_slices: slices must be 0 (automatic) or 1 .. 64");
  JH_REQUIRE(max_workgroups >= 0, "model_set_rollout_slices: max_workgroups must be 0 (the resident slots) or a positive cap on the queue's grid");
  JH_REQUIRE((flags & ~1) == 0, "model_set_rollout_slices: flags has bit 0 (every hand-off counts as missed) and no other");
  m->rollout_slices = slices; m->rollout_max_workgroups = max_workgroups; m->rollout_slice_flags = flags;
  m->rollout_nbounds = 0;  // (the later call decides: an explicit schedule set before is gone)
  return JH_OK;
}

extern "C" int jh_model_set_rollout_slice_bounds(jh_model* m, const int* first_steps, int n) {
  JH_REQUIRE(m != nullptr && n >= 0 && n <= JH_MAX_SLICE_BOUNDS && (n == 0 || first_steps != nullptr), "model_set_rollout_slice_bounds: 0 (none) to %d first steps", JH_MAX_SLICE_BOUNDS);
  for (int i = 0; i < n; i++)
    JH_REQUIRE(first_steps[i] > (i ? first_steps[i - 1] : 0), "model_set_rollout_slice_bounds: first steps must be positive and strictly increasing (entry %d is %d)", i, first_steps[i]);
  for (int i = 0; i < n; i++) m->rollout_bounds[i] = first_steps[i];
  m->rollout_nbounds = n;
  if (n > 0) m->rollout_slices = 0;  // (the later call decides: a forced number of equal slices is gone; the grid's cap and the flags stay)
  return JH_OK;
}

extern "C" int jh_model_last_rollout_slice_bounds(const jh_model* m, int* out, int cap) {
  JH_REQUIRE(m != nullptr && cap >= 0 && (cap == 0 || out != nullptr), "model_last_rollout_slice_bounds: null model or output");
  const int n = __atomic_load_n(&m->last_rollout_nbounds, __ATOMIC_RELAXED);
  for (int i = 0; i < n && i < cap; i++) out[i] = __atomic_load_n(&m->last_rollout_bounds[i], __ATOMIC_RELAXED);
  return n;
}

void jh_model_note_slice_bounds(const jh_model* m, int slices, int H, const int* bounds) {
  const int n = slices > 1 ? (slices - 1 < 63 ? slices - 1 : 63) : 0;
  for (int i = 0; i < n; i++) __atomic_store_n(&m->last_rollout_bounds[i], bounds ? bounds[i] : (i + 1) * H / slices, __ATOMIC_RELAXED);
  __atomic_store_n(&m->last_rollout_nbounds, n, __ATOMIC_RELAXED);
}

// The automatic schedule of the leap queue's horizon slices, a pure function of the launch's shape (profiles/leap_tapered_slices.md).  Below two groups per wave slot: whole
// groups (a slice's producer must as good as always have parked its state by the time the slice is drawn).  From two: four equal slices.  From JH_TAPER_DEPTH groups per slot
// and JH_TAPER_MIN_H steps: slices that shorten towards the end of the horizon -- 3/8, 1/4, 3/16, 1/8 and 1/16 of it, 24 / 16 / 12 / 8 / 4 steps of 64 -- so that the tickets
// drawn last, over which the launch drains, are the short ones; one hand-off more than the equal slices.  The depth condition: a missed hand-off of the last slice recomputes
// fifteen sixteenths of the horizon, which would undo the gain in the launch's tail.
#ifndef JH_AUTO_TAPER
#define JH_AUTO_TAPER 1
#endif
constexpr int JH_TAPER_DEPTH = 4, JH_TAPER_MIN_H = 32;
extern "C" int jh_rollout_slice_schedule(int H, int groups, int wave_slots, int* first_steps, int cap) {
  JH_REQUIRE(H >= 0 && groups >= 0 && wave_slots >= 0 && cap >= 0 && (cap == 0 || first_steps != nullptr), "rollout_slice_schedule: negative argument or null output");
  int b[4], n = 0;
  if (wave_slots > 0 && (long long)groups >= 2ll * wave_slots) {
    if (JH_AUTO_TAPER && H >= JH_TAPER_MIN_H && (long long)groups >= (long long)JH_TAPER_DEPTH * wave_slots) {
      const long long num[4] = {6, 10, 13, 15};
      for (n = 0; n < 4; n++) b[n] = (int)(num[n] * H / 16);
    } else {
      const int S = H < 4 ? H : 4;
      for (int i = 1; i < S; i++) b[n++] = i * H / S;
    }
  }
  for (int i = 0; i < n && i < cap; i++) first_steps[i] = b[i];
  return n;
}

extern "C" int jh_model_last_rollout_slices(const jh_model* m) {
  JH_REQUIRE(m != nullptr, "model_last_rollout_slices: null model");
  return __atomic_load_n(&m->last_rollout_slices, __ATOMIC_RELAXED);
}

extern "C" int jh_model_recomputed_units(jh_model* m) {
  JH_REQUIRE(m != nullptr, "model_recomputed_units: null model");
  int v = 0;
  JH_HIP(hipMemcpy(&v, m->d_stats + JH_STAT_RECOMPUTED, sizeof(int), hipMemcpyDeviceToHost));
  return v;
}

extern "C" int jh_upload_async(void* dst, const void* src, size_t nbytes, void* stream) {
  JH_REQUIRE(dst && src, "upload_async: null pointer");
  JH_HIP(hipMemcpyAsync(dst, src, nbytes, hipMemcpyHostToDevice, (hipStream_t)stream));
  return JH_OK;
}

extern "C" int jh_download_wait(void* dst, const void* src, size_t nbytes, void* stream) {
  JH_REQUIRE(dst && src, "download_wait: null pointer");
  JH_HIP(hipMemcpyAsync(dst, src, nbytes, hipMemcpyDeviceToHost, (hipStream_t)stream));
  JH_HIP(hipStreamSynchronize((hipStream_t)stream));
  return JH_OK;
}

// One completion mark per (host thread, stream): an event belongs to the device it was created on, so a thread that drives controllers on several GPUs
// (one stream each) needs one per stream, created with that stream's device current.  `end` waits for the marks in the order they were set.
namespace {
struct DlMark { void* stream; hipEvent_t ev; };
thread_local std::vector<DlMark> g_dl_marks;     // events owned by this thread, one per stream it has downloaded on
struct DlPending { hipEvent_t ev; const unsigned* flag; unsigned expect; };  // flag non-null: a word in pinned host memory the last workgroup of the update sets (jh_plan_step)
thread_local std::vector<DlPending> g_dl_pending;  // marks set by `begin` and not yet waited for, oldest first
}  // namespace

static int download_begin(void* dst, const void* src, size_t nbytes, void* stream, const unsigned* flag, unsigned expect) {
  JH_REQUIRE(dst && src, "download_begin: null pointer");
  hipEvent_t ev = nullptr;
  for (const DlMark& mk : g_dl_marks) if (mk.stream == stream) ev = mk.ev;
  if (!ev) {
    int cur = 0, dev = 0;
    JH_HIP(hipGetDevice(&cur));
    dev = cur;
    if (stream) { hipDevice_t sd; if (hipStreamGetDevice((hipStream_t)stream, &sd) == hipSuccess) dev = (int)sd; else (void)hipGetLastError(); }
    if (dev != cur) JH_HIP(hipSetDevice(dev));
    hipError_t e = hipEventCreateWithFlags(&ev, hipEventDisableTiming);
    if (dev != cur) (void)hipSetDevice(cur);
    JH_HIP(e);
    g_dl_marks.push_back({stream, ev});
  }
  if (nbytes > 0) JH_HIP(hipMemcpyAsync(dst, src, nbytes, hipMemcpyDeviceToHost, (hipStream_t)stream));  // (0 bytes: the kernels wrote the pinned host block themselves; the mark alone)
  JH_HIP(hipEventRecord(ev, (hipStream_t)stream));
  g_dl_pending.push_back({ev, flag, expect});
  return JH_OK;
}

extern "C" int jh_download_begin(void* dst, const void* src, size_t nbytes, void* stream) { return download_begin(dst, src, nbytes, stream, nullptr, 0u); }

extern "C" int jh_download_end(void) {
  JH_REQUIRE(!g_dl_pending.empty(), "download_end without download_begin");
  const DlPending pd = g_dl_pending.front();
  g_dl_pending.erase(g_dl_pending.begin());
  if (pd.flag) {
    // The update's last workgroup stored `expect` behind its results (system-scope release): the host sees them some microseconds before the stream's event -- the kernel's
    // end-of-launch write-back, the marker packet and its signal -- would report.  The event is looked at every few thousand polls so that a launch that died cannot hang the host.
    for (unsigned spin = 1;; spin++) {
      if (__atomic_load_n(pd.flag, __ATOMIC_ACQUIRE) == pd.expect) return JH_OK;
      __builtin_ia32_pause();
      if ((spin & 0x3FFFu) == 0u) {
        const hipError_t q = hipEventQuery(pd.ev);
        if (q == hipSuccess) { if (__atomic_load_n(pd.flag, __ATOMIC_ACQUIRE) != pd.expect) { jh_set_error("download_end: the launch finished without setting its completion flag"); return JH_ERR_HIP; } return JH_OK; }
        if (q != hipErrorNotReady) JH_HIP(q);
      }
    }
  }
  JH_HIP(hipEventSynchronize(pd.ev));
  return JH_OK;
}

extern "C" int jh_model_profile(jh_model* m, long long* out /* 10 phase cycle totals; zero unless the kernel was built with its phase clock (JH_V6_PHASES) */) {
  JH_REQUIRE(m && out, "model_profile: null pointer");
  JH_HIP(hipMemcpy(out, m->d_stats + 4, 10 * sizeof(long long), hipMemcpyDeviceToHost));
  return JH_OK;
}

// One fused launch on the record: the argument checks, then the model's build, else the cross-check library.
static int rollout_cost(const jh_model* m, const jh_rollout_args& a, void* stream) {
  JH_REQUIRE(m && a.x0 && a.nominal && a.noise && a.sigma && a.W && a.lohi && a.tp && a.costs, "rollout_cost: null pointer");
  if (a.trace) JH_REQUIRE(trace_layout(m).floats > 0, "rollout_cost_traced: this model's fused kernel writes no trace sensors (jh_model_trace_layout)");
  JH_REQUIRE(a.N > 0 && a.H > 0 && a.K >= 1, "rollout_cost: N, H, K must be positive (N=%d H=%d K=%d)", a.N, a.H, a.K);
  JH_REQUIRE(a.ldn >= a.N, "rollout_cost: ldn (%d) < N (%d)", a.ldn, a.N);
  JH_REQUIRE(a.K * m->nu <= JH_MAX_KNOT_DIM, "rollout_cost: K*nu = %d exceeds %d", a.K * m->nu, JH_MAX_KNOT_DIM);
  JH_REQUIRE(a.n_offset >= 0, "rollout_cost: negative n_offset");
  hipStream_t st = (hipStream_t)stream;
  if (const jh_engine_build* eb = engine_build(m)) return eb->rollout_cost(m, a, st);
  JH_REQUIRE(a.trace == nullptr, "rollout_cost_traced: only the product kernels (generation 3, cartpole, cylinder_push) write trace sensors");
  if (!g_xcheck.rollout_cost) { jh_set_error("rollout_cost: no kernel for this model / generation in this library"); return JH_ERR_UNSUPPORTED; }
  return g_xcheck.rollout_cost(m, m->kernel_gen, a.x0, a.nominal, a.noise, a.ldn, a.sigma, a.W, a.lohi, a.tp, a.phase, a.N, a.n_offset, a.H, a.K, a.costs, a.knots_out, stream);
}

extern "C" int jh_rollout_cost_traced(const jh_model* m, const float* x0, const float* nominal, const float* noise, int ldn, const float* sigma,
                                      const float* W, const float* lohi, const float* tp, int phase, int N, int n_offset, int H, int K, float* costs,
                                      float* knots_out, float* trace, void* stream) {
  const jh_rollout_args a = {x0, nominal, noise, ldn, sigma, W, lohi, tp, phase, N, n_offset, H, K, costs, knots_out, trace};
  return rollout_cost(m, a, stream);
}

extern "C" int jh_rollout_cost(const jh_model* m, const float* x0, const float* nominal, const float* noise, int ldn, const float* sigma,
                               const float* W, const float* lohi, const float* tp, int phase, int N, int n_offset, int H, int K, float* costs,
                               float* knots_out, void* stream) {
  return jh_rollout_cost_traced(m, x0, nominal, noise, ldn, sigma, W, lohi, tp, phase, N, n_offset, H, K, costs, knots_out, nullptr, stream);
}

// Closed-form models (cartpole, cylinder_push): the rollout kernels are ~50 us, so a second launch and the gap in front of it are a fifth of the plan step -- the two run as
// one launch (jh_simple.hip) wherever its LDS staging fits (K <= jh_model_one_launch_max_knots).  jh_model_set_plan_step_launches forces either form (2: the rollout kernel,
// then k_update_tail), so that tests/test_gpu_plan_edges.py compares the two bit for bit in one process; JUDO_AMD_PLAN_STEP_LAUNCHES=2 sets that for every new model.
// Forced one launch where it cannot run (knots_out requested, or K above the limit) is an error, not a quiet switch.
static int plan_step_launches(const jh_model* m, int N, int H, int K, const float* costs, const float* knots_out, const float* W, const float* noise, int ldn, bool* one) {
  *one = false;
  const jh_engine_build* eb = engine_build(m);
  if (m->plan_step_launches == 2 || !(eb && eb->plan_step)) return JH_OK;
  const bool fits = costs && W && noise && N > 0 && H > 0 && K >= 1 && ldn >= N && K * m->nu <= JH_MAX_KNOT_DIM && K <= eb->one_launch_max_knots(m, H);
  if (m->plan_step_launches == 1) {
    JH_REQUIRE(!knots_out, "plan_step: the one-launch plan step writes no candidate knots (knots_out), and one launch is forced (jh_model_set_plan_step_launches)");
    JH_REQUIRE(fits, "plan_step: one launch is forced but K = %d exceeds its LDS staging at H = %d (jh_model_one_launch_max_knots)", K, H);
  }
  *one = fits && !knots_out;
  if (*one) __atomic_fetch_add(&m->one_launch_steps, 1, __ATOMIC_RELAXED);
  return JH_OK;
}

// What every plan step does around its launches, written once.
// The completion mark: `out_host_mark` other than `out` (and not null) is a 4-byte word in device-visible pinned host memory -- the update's last workgroup stores its old
// value + 1 there behind the results, and jh_download_end polls it; out_host_mark == out (or null): the stream's event alone.
struct jh_step_mark { unsigned* flag; unsigned expect; };
static jh_step_mark step_mark(void* out_host_mark, const float* out) {
  unsigned* flag = (out_host_mark && out_host_mark != (const void*)out) ? (unsigned*)out_host_mark : nullptr;
  return {flag, flag ? __atomic_load_n(flag, __ATOMIC_RELAXED) + 1u : 0u};
}
// The front: the packed block(s) go up -- unless blk_dev == blk_host, a device-visible pinned host block the kernels read in place (the closed-form models: a few hundred
// bytes read once per workgroup cost less than the copy in front of the launch) --, then timing[0].
static int step_begin(void* blk_dev, const void* blk_host, size_t bytes, void* const* timing, void* stream) {
  if (blk_dev != blk_host) { if (int rc = jh_upload_async(blk_dev, blk_host, bytes, stream)) return rc; }
  if (timing) JH_HIP(hipEventRecord((hipEvent_t)timing[0], (hipStream_t)stream));
  return JH_OK;
}
// The end, if the launches went out (`rc`): timing[2], then the mark behind `out` (null: the shard form, which has none).
static int step_end(int rc, float* out, const jh_step_mark& mk, void* const* timing, void* stream) {
  if (rc == JH_OK && timing) JH_HIP(hipEventRecord((hipEvent_t)timing[2], (hipStream_t)stream));
  if (rc == JH_OK && out) rc = download_begin(out, out, 0, stream, mk.flag, mk.expect);
  return rc;
}

// One plan-step iteration as ONE call (Controller.update_action's loop body, judo/controller/controller.py:250-299): the packed host block x0 | nominal | sigma |
// task params | bounds goes up, the fused rollout + cost kernel runs, and the update's tail reduces the costs.  Everything is enqueued on `stream`; nothing is waited for
// here.  Five ctypes calls less per plan step than the separate entry points: a tenth of a small one.  The tail writes one of two destinations:
//  - `out` (jh_plan_step): nominal | sigma | trace records, normally the pinned host block itself, then the completion mark of jh_download_begin, which
//    jh_download_end waits for (`out_host_mark`: step_mark above);
//  - `rec_out` (jh_plan_step_shard): this rank's RECORD (jh_update_shard's) instead of the nominal, and no mark: the caller all-gathers the G records and
//    jh_plan_merge finishes the update.
static int plan_step(const char* who, const jh_model* m, void* blk_dev, const void* blk_host, size_t blk_bytes, int o_nominal, int o_sigma, int o_tp, int o_lohi,
                     const float* noise, int ldn, const float* W, int phase, int N, int n_offset, int H, int K, float* costs, float* knots_out, float* trace, int mode,
                     float lambda, int k, int tie_high, int E, int row_floats, int colmajor, float* scratch, float* out, void* out_host_mark, float* rec_out,
                     void* const* timing, void* stream) {
  JH_REQUIRE(m && blk_dev && blk_host && (out || rec_out) && scratch, "%s: null pointer", who);
  const float* b = (const float*)blk_dev;
  hipStream_t st = (hipStream_t)stream;
  int rc = step_begin(blk_dev, blk_host, blk_bytes, timing, stream);
  const int KU = K * m->nu;
  const jh_step_mark mk = step_mark(out_host_mark, out);
  bool one = false;
  if (rc == JH_OK) rc = plan_step_launches(m, N, H, K, costs, knots_out, W, noise, ldn, &one);
  // two launches: the rollout kernel, then k_update_tail; one (closed-form models): rollout + cost + the update's tail in jh_simple.hip's k_plan_step, where the
  // rollout / update split of the timing events collapses
  const jh_rollout_args ra = {b, b + o_nominal, noise, ldn, b + o_sigma, W, b + o_lohi, b + o_tp, phase, N, n_offset, H, K, costs, knots_out, trace};
  if (rc == JH_OK && !one) rc = rollout_cost(m, ra, stream);
  if (rc == JH_OK && !one && timing) JH_HIP(hipEventRecord((hipEvent_t)timing[1], st));
  jh_upd::TailArgs a;
  if (rc == JH_OK)
    rc = jh_update_tail_args(who, costs, nullptr, b + o_nominal, noise, ldn, b + o_sigma, b + o_lohi, N, n_offset, K, m->nu, mode, lambda, k, tie_high, trace ? E : 0, trace, row_floats,
                             colmajor, scratch, out, out ? out + KU : nullptr, (out && trace && E > 0) ? out + 2 * KU : nullptr, rec_out, &a);
  a.done_flag = mk.flag; a.done_value = mk.expect;
  if (rc == JH_OK) rc = one ? engine_build(m)->plan_step(m, b, W, b + o_tp, H, K, a, st) : jh_update_tail_launch(a, st);
  if (rc == JH_OK && one && timing) JH_HIP(hipEventRecord((hipEvent_t)timing[1], st));
  return step_end(rc, out, mk, timing, stream);
}

extern "C" int jh_plan_step(const jh_model* m, void* blk_dev, const void* blk_host, size_t blk_bytes, int o_nominal, int o_sigma, int o_tp, int o_lohi, const float* noise, int ldn,
                            const float* W, int phase, int N, int n_offset, int H, int K, float* costs, float* knots_out, float* trace, int mode, float lambda, int k, int tie_high, int E,
                            int row_floats, int colmajor, float* scratch, float* out, void* out_host_mark, void* const* timing /* 3 events of jh_event_create, or NULL */, void* stream) {
  JH_REQUIRE(out, "plan_step: null pointer");
  return plan_step("plan_step", m, blk_dev, blk_host, blk_bytes, o_nominal, o_sigma, o_tp, o_lohi, noise, ldn, W, phase, N, n_offset, H, K, costs, knots_out, trace, mode, lambda, k,
                   tie_high, E, row_floats, colmajor, scratch, out, out_host_mark, nullptr, timing, stream);
}

// The B phase words of a batched fr3_pick call (`what`: whose, for the message), on the host, before anything is enqueued: the kernel converts the word and branches on it.
static int phase_words(const char* who, const char* what, int B, const void* blk_host, size_t blk_bytes, size_t blk_stride_bytes, int o_phase) {
  JH_REQUIRE(sizeof(float) * ((size_t)o_phase + 1) <= blk_bytes, "%s: o_phase = %d lies outside a block of %zu bytes", who, o_phase, blk_bytes);
  for (int p = 0; p < B; p++) {
    const float w = reinterpret_cast<const float*>(static_cast<const char*>(blk_host) + (size_t)p * blk_stride_bytes)[o_phase];
    JH_REQUIRE(w == 0.f || w == 1.f || w == 2.f || w == 3.f, "%s: the phase word of %s %d is %g, not exactly 0, 1, 2 or 3 (LIFT, MOVE, PLACE, HOMING)", who, what, p, (double)w);
  }
  return JH_OK;
}

// What a packed block holds and, where every problem (or controller) has a block and a noise matrix of its own (`batched`), what lies between two of them: the checks of
// every plan step with a problem axis, in one place.  (The output stride stays with the caller: the size of its record depends on the trace arguments.)
struct jh_block_shape {
  size_t bytes; int o_nominal, o_sigma, o_tp, o_lohi;  // a block's size; the float offsets of nominal | sigma | task params | bounds in it (x0 stands at 0)
  int ldn, N, H, K;
  bool batched = false; size_t stride_bytes = 0, noise_stride_floats = 0;
};
static int check_block_shape(const char* who, const jh_model* m, const jh_block_shape& s) {
  JH_REQUIRE(s.N > 0 && s.H > 0 && s.K >= 1, "%s: N, H, K must be positive (N=%d H=%d K=%d)", who, s.N, s.H, s.K);
  JH_REQUIRE(s.ldn >= s.N, "%s: ldn (%d) < N (%d)", who, s.ldn, s.N);
  const int KU = s.K * m->nu, nx = m->nq + m->nv;
  JH_REQUIRE(KU <= JH_MAX_KNOT_DIM, "%s: K*nu = %d exceeds %d", who, KU, JH_MAX_KNOT_DIM);
  JH_REQUIRE(s.o_nominal >= 0 && s.o_sigma >= 0 && s.o_tp >= 0 && s.o_lohi >= 0, "%s: negative block offset", who);
  const size_t need = sizeof(float) * (size_t)std::max(std::max(nx, s.o_nominal + KU), std::max(std::max(s.o_sigma + KU, s.o_tp + m->ntaskparam), s.o_lohi + 2 * m->nu));
  JH_REQUIRE(s.bytes >= need, "%s: a block of %zu bytes does not hold x0 | nominal | sigma | task params | bounds at the given offsets (%zu bytes)", who, s.bytes, need);
  if (!s.batched) return JH_OK;
  JH_REQUIRE(s.stride_bytes >= s.bytes && s.stride_bytes % sizeof(float) == 0, "%s: blk_stride_bytes = %zu is smaller than a block (%zu bytes) or no multiple of 4", who, s.stride_bytes, s.bytes);
  JH_REQUIRE(s.noise_stride_floats >= (size_t)KU * (size_t)s.ldn, "%s: noise_stride_floats = %zu is smaller than a problem's noise (K*nu*ldn = %zu)", who, s.noise_stride_floats, (size_t)KU * (size_t)s.ldn);
  return JH_OK;
}

// B plan steps of one model as ONE call (include/judo_amd.h): the B packed blocks go up in one copy (or are read in place), the kernels take the problem from blockIdx.y and
// reach its buffers through strides, and one completion mark stands behind all of them.  Problem 0's launch record is built by the single call's own checks
// (jh_update_tail_args); the kernels derive problem b's from it.  `images` / `image_stride`: the float section the rollout kernels read for problem 0 and the floats to
// problem b + 1's from problem b's -- m->d_f and 0 for jh_plan_step_batch, a model set's buffer and stride for jh_plan_step_batch_models: one code path.  `ints`: the int
// section the leap kernel reads -- m->d_i, or a model set's copy without pair tables.  The record is jh_set_step's sibling (below): what the four entries share.
struct jh_batch_step {
  const char* who; const jh_model* m; const float* images; long long image_stride; const int* ints; int B;
  void* blk_dev; const void* blk_host; jh_block_shape shape; const float *noise, *W;  // the B blocks (blk_dev == blk_host: read in place, as jh_plan_step), their shape and strides, noise and spline weights
  float *costs, *trace; int mode; float lambda; int k, tie_high, E, row_floats, colmajor;  // the update and its trace records
  float *scratch, *out; size_t out_stride_floats; void* out_host_mark; void* const* timing; void* stream;
  int o_phase = -1;  // the float offset of every block's phase word (jh_plan_step_batch_phases, fr3_pick alone), or -1: an entry without one, which keeps refusing fr3_pick
};

static int plan_step_batch(const jh_batch_step& r) {
  const char* who = r.who;
  const jh_model* m = r.m;
  const jh_block_shape& d = r.shape;
  const int B = r.B, N = d.N, H = d.H, K = d.K;
  JH_REQUIRE(m && r.blk_dev && r.blk_host && r.out && r.scratch && r.noise && r.W && r.costs, "%s: null pointer", who);
  if (m->kind == JH_TASK_FR3_PICK && r.o_phase < 0) { jh_set_error("%s: fr3_pick has no batched plan step (its phase is chosen per problem on the host) behind this entry: jh_plan_step_batch_phases takes a phase word per problem, jh_plan_step_batch_phases_models a set of fr3_pick models as well", who); return JH_ERR_UNSUPPORTED; }
  if (m->kind != JH_TASK_FR3_PICK && r.o_phase >= 0) { jh_set_error("%s: a phase word per problem is fr3_pick's alone; jh_plan_step_batch plans this model", who); return JH_ERR_UNSUPPORTED; }
  if (m->kind == JH_TASK_LEAP_CUBE && m->kernel_gen != 3) { jh_set_error("%s: only kernel generation 3 of the leap family has a batched launch (this model runs %d)", who, m->kernel_gen); return JH_ERR_UNSUPPORTED; }
  JH_REQUIRE(B >= 1, "%s: B must be at least 1 (B=%d)", who, B);
  JH_REQUIRE(B <= 65535, "%s: B = %d exceeds the 65535 problems of a launch (the grid's second dimension)", who, B);
  JH_REQUIRE(r.o_phase < 0 || K <= 8, "%s: the cooperative arm kernel keeps at most 8 knots per actuator in registers (K=%d)", who, K);
  if (int rc = check_block_shape(who, m, d)) return rc;
  const int KU = K * m->nu;
  if (r.trace) { const int t_nfl = trace_layout(m).floats; JH_REQUIRE(t_nfl > 0 && r.row_floats == H * t_nfl, "%s: row_floats = %d is not H x the model's %d trace floats per step (jh_model_trace_layout)", who, r.row_floats, t_nfl); }
  const int E_t = r.trace ? r.E : 0;
  JH_REQUIRE(E_t >= 0 && E_t <= JH_MAX_ELITES, "%s: bad trace arguments (E=%d)", who, r.E);
  const size_t rec = 2 * (size_t)KU + (size_t)E_t * (2 + (size_t)(E_t > 0 ? r.row_floats : 0));
  JH_REQUIRE(r.out_stride_floats >= rec, "%s: out_stride_floats = %zu is smaller than an output record (nominal | sigma | E trace records = %zu floats)", who, r.out_stride_floats, rec);
  const jh_engine_build* eb = engine_build(m);
  if (!(eb && eb->rollout_cost_batch)) { jh_set_error("%s: no batched kernel for this model", who); return JH_ERR_UNSUPPORTED; }
  if (r.o_phase >= 0) { if (int rc = phase_words(who, "problem", B, r.blk_host, d.bytes, d.stride_bytes, r.o_phase)) return rc; }
  hipStream_t st = (hipStream_t)r.stream;
  const float* b = (const float*)r.blk_dev;
  if (int rc = step_begin(r.blk_dev, r.blk_host, (size_t)(B - 1) * d.stride_bytes + d.bytes, r.timing, r.stream)) return rc;
  const jh_step_mark mk = step_mark(r.out_host_mark, r.out);
  bool one = false;
  if (int rc = plan_step_launches(m, N, H, K, r.costs, nullptr, r.W, r.noise, d.ldn, &one)) return rc;
  jh_upd::TailArgs a;
  if (int rc = jh_update_tail_args(who, r.costs, nullptr, b + d.o_nominal, r.noise, d.ldn, b + d.o_sigma, b + d.o_lohi, N, 0, K, m->nu, r.mode, r.lambda, r.k, r.tie_high, E_t, r.trace, r.row_floats,
                                   r.colmajor, r.scratch, r.out, r.out + KU, E_t > 0 ? r.out + 2 * KU : nullptr, nullptr, &a)) return rc;
  jh_upd::BatchArgs s;
  s.B = B; s.blk = (long long)(d.stride_bytes / sizeof(float)); s.noise = (long long)d.noise_stride_floats; s.costs = N; s.trace = (long long)N * r.row_floats;
  s.scratch = (long long)jh_update_fused_scratch_floats(N, K, m->nu); s.out = (long long)r.out_stride_floats;
  s.counter = reinterpret_cast<unsigned*>(r.scratch) + 1; s.done_flag = mk.flag; s.done_value = mk.expect; s.image = r.image_stride;
  int rc = JH_OK;
  if (one) rc = eb->plan_step_batch(m, r.images, b, r.W, b + d.o_tp, H, K, a, s, st);
  else {
    const jh_rollout_args ra = {b, b + d.o_nominal, r.noise, d.ldn, b + d.o_sigma, r.W, b + d.o_lohi, b + d.o_tp, 0, N, 0, H, K, r.costs, nullptr, r.trace};
    jh_rollout_batch rb = {r.images, r.image_stride, r.ints, B, s.blk, s.noise};
    rb.o_phase = r.o_phase;
    rc = eb->rollout_cost_batch(m, ra, rb, st);
    if (rc == JH_OK && r.timing) JH_HIP(hipEventRecord((hipEvent_t)r.timing[1], st));
    if (rc == JH_OK) rc = jh_update_tail_batch_launch(a, s, st);
  }
  if (rc == JH_OK && one && r.timing) JH_HIP(hipEventRecord((hipEvent_t)r.timing[1], st));
  return step_end(rc, r.out, mk, r.timing, r.stream);
}

// The entries: their own pre-checks, then the record.  (`JH_BATCH_STEP`: the fields every entry has, in the record's order.)
#define JH_BATCH_STEP(who, m, images, image_stride, ints, B)                                                                                                               \
  {who, m, images, image_stride, ints, B, blk_dev, blk_host, {blk_bytes, o_nominal, o_sigma, o_tp, o_lohi, ldn, N, H, K, true, blk_stride_bytes, noise_stride_floats}, noise, W, \
   costs, trace, mode, lambda, k, tie_high, E, row_floats, colmajor, scratch, out, out_stride_floats, out_host_mark, timing, stream}

extern "C" int jh_plan_step_batch(const jh_model* m, int B, void* blk_dev, const void* blk_host, size_t blk_bytes, size_t blk_stride_bytes, int o_nominal, int o_sigma, int o_tp, int o_lohi,
                                  const float* noise, int ldn, size_t noise_stride_floats, const float* W, int N, int H, int K, float* costs, float* trace, int mode, float lambda, int k,
                                  int tie_high, int E, int row_floats, int colmajor, float* scratch, float* out, size_t out_stride_floats, void* out_host_mark, void* const* timing,
                                  void* stream) {
  JH_REQUIRE(m != nullptr, "plan_step_batch: null pointer");
  return plan_step_batch(JH_BATCH_STEP("plan_step_batch", m, m->d_f, 0, m->d_i, B));
}

// jh_plan_step_batch for fr3_pick (include/judo_amd.h): the same code path with a phase word in every problem's block.
extern "C" int jh_plan_step_batch_phases(const jh_model* m, int B, void* blk_dev, const void* blk_host, size_t blk_bytes, size_t blk_stride_bytes, int o_nominal, int o_sigma, int o_tp, int o_lohi,
                                         int o_phase, const float* noise, int ldn, size_t noise_stride_floats, const float* W, int N, int H, int K, float* costs, float* trace, int mode,
                                         float lambda, int k, int tie_high, int E, int row_floats, int colmajor, float* scratch, float* out, size_t out_stride_floats, void* out_host_mark,
                                         void* const* timing, void* stream) {
  JH_REQUIRE(m != nullptr, "plan_step_batch_phases: null pointer");
  JH_REQUIRE(o_phase >= 0, "plan_step_batch_phases: negative block offset (o_phase=%d)", o_phase);
  jh_batch_step r = JH_BATCH_STEP("plan_step_batch_phases", m, m->d_f, 0, m->d_i, B);
  r.o_phase = o_phase;
  return plan_step_batch(r);
}

// ---- model sets: B images of one model's float section in one device buffer, a fixed stride apart (include/judo_amd.h) ----
// Everything but the float section is member 0's: the launchers read its int section, its settings and its counters, so a member must agree with it on all of them.
struct jh_model_set {
  int B;
  size_t nf, stride;                   // floats per image; floats from one image to the next (nf rounded up to a multiple of 64)
  float* d_images;                     // B x stride floats on member 0's device
  const jh_model* m0;                  // member 0: the int section, the dimensions, the kernel build and settings, d_stats
  std::vector<std::vector<float>> hf;  // host copies of the members' float sections (jh_model_set_info: how many differ from member 0's)
  std::vector<std::vector<int>> hi;    // ... and of their int sections (they differ in the pair tables at most)
  int* d_i_plain;                      // member 0's int section with the pair tables' header slot zeroed: what the launch reads when the members cannot share the tables
  bool tables;                         // every member may share member 0's pair tables (pair_tables_shared)
};

// The int sections of two members of a set agree but for the pair tables' block, which `pair_tables_shared` weighs: the word where they differ, or -1.
static long int_sections_differ(const std::vector<int>& a, const std::vector<int>& b) {
  if (a.size() != b.size()) return 0;
  const long o = a.size() > (size_t)HI_PT && a[HI_PT] == b[HI_PT] && a[HI_PT] > 0 ? a[HI_PT] : -1;
  for (long w = 0; w < (long)a.size(); w++) if (a[w] != b[w] && !(o >= 0 && w >= o && w < o + JH_PT_LEN)) return w;
  return -1;
}

// (Re)derive what follows from the members: whether they share the pair tables, and the int section without them.
static int model_set_tables(jh_model_set* s, bool member0_changed) {
  s->tables = true;
  if (s->m0->kind == JH_TASK_FR3_PICK) return JH_OK;  // (no pair tables: the members' int sections are member 0's word for word, and the launch reads m0->d_i)
  jh_eng::HostImage lead;
  lead.bind(s->hf[0].data(), s->hi[0].data(), s->hf[0].size(), s->hi[0].size());
  for (int b = 1; b < s->B && s->tables; b++) {
    jh_eng::HostImage member;
    member.bind(s->hf[b].data(), s->hi[b].data(), s->hf[b].size(), s->hi[b].size());
    s->tables = jh_eng::pair_tables_shared(lead, member);
  }
  if (!member0_changed) return JH_OK;  // (the int section without tables is member 0's: uploaded when the set is made and when member 0 is replaced)
  std::vector<int> plain = s->hi[0];
  if (plain.size() > (size_t)HI_PT) plain[HI_PT] = 0;
  if (!plain.empty()) JH_HIP(hipMemcpy(s->d_i_plain, plain.data(), 4 * plain.size(), hipMemcpyHostToDevice));
  return JH_OK;
}

// May `m` be member `b` of a set whose member 0 is `m0` (b == 0: may `m` lead a set)?  JH_OK, or the status with the error set: it names the member and the field.
// `fr3`: the set is one of fr3_pick models (jh_fr3_model_set_create), which the phase-taking entries plan; every other set keeps refusing the family.
static int model_set_member(const char* who, const jh_model* m0, const jh_model* m, int b, bool fr3) {
  JH_REQUIRE(m != nullptr, "%s: member %d is a null pointer", who, b);
  if (m->kind == JH_TASK_FR3_PICK && !fr3) {
    jh_set_error("%s: member %d is an fr3_pick model, which has no batched plan step (its phase is chosen per problem on the host) behind the entries that take this set.  "
                 "jh_fr3_model_set_create makes a set of fr3_pick models for jh_plan_step_batch_phases_models and jh_plan_step_randomized_phase", who, b);
    return JH_ERR_UNSUPPORTED;
  }
  if (m->kind != JH_TASK_FR3_PICK && fr3) { jh_set_error("%s: member %d is no fr3_pick model (kind %d): this set holds fr3_pick models alone; jh_model_set_create makes a set of every other family", who, b, m->kind); return JH_ERR_UNSUPPORTED; }
  if (m->kind == JH_TASK_LEAP_CUBE && m->kernel_gen != 3) { jh_set_error("%s: member %d runs kernel_gen %d: only kernel generation 3 of the leap family has a batched launch", who, b, m->kernel_gen); return JH_ERR_UNSUPPORTED; }
  if (m->kind == JH_TASK_FR3_PICK && m->kernel_gen != 3) { jh_set_error("%s: member %d runs kernel_gen %d: only kernel generation 3 of fr3_pick has a batched launch", who, b, m->kernel_gen); return JH_ERR_UNSUPPORTED; }
  if (const jh_engine_build* eb = engine_build(m); !(eb && eb->rollout_cost_batch)) { jh_set_error("%s: member %d: no batched kernel for this model (kind %d)", who, b, m->kind); return JH_ERR_UNSUPPORTED; }
  if (m != m0) {
#define JH_SET_SAME(field, fmt)                                                                                                                                    \
  JH_REQUIRE(m->field == m0->field, "%s: member %d differs from the set's member 0 in " #field " (" fmt " against " fmt ")", who, b, m->field, m0->field)
    JH_SET_SAME(device, "%d"); JH_SET_SAME(kind, "%d"); JH_SET_SAME(nq, "%d"); JH_SET_SAME(nv, "%d"); JH_SET_SAME(nu, "%d"); JH_SET_SAME(ns, "%d"); JH_SET_SAME(ntaskparam, "%d");
    JH_SET_SAME(nf, "%zu"); JH_SET_SAME(ni, "%zu");
    if (const long w = int_sections_differ(m->h_i, m0->h_i); w >= 0) {
      jh_set_error("%s: member %d differs from the set's member 0 in the int section h_i (word %ld: %d against %d): topology, pair lists and lane lists are one for the launch", who, b, w, m->h_i[w], m0->h_i[w]);
      return JH_ERR_INVALID;
    }
    JH_SET_SAME(kernel_gen, "%d"); JH_SET_SAME(contact_capacity, "%d"); JH_SET_SAME(cylinders, "%d"); JH_SET_SAME(arm_pairs, "%d"); JH_SET_SAME(self_collision, "%d"); JH_SET_SAME(rollout_schedule, "%d");
    JH_SET_SAME(rollout_slices, "%d"); JH_SET_SAME(rollout_nbounds, "%d");
    for (int i = 0; i < m0->rollout_nbounds; i++) JH_SET_SAME(rollout_bounds[i], "%d");
 JH_SET_SAME(rollout_max_workgroups, "%d"); JH_SET_SAME(rollout_slice_flags, "%d");
    JH_SET_SAME(plan_step_launches, "%d");
#undef JH_SET_SAME
  }
  JH_REQUIRE(m->h_f.size() == m->nf && m->d_f, "%s: member %d has no float section of nf = %zu floats", who, b, m->nf);
  if (m->kind == JH_TASK_LEAP_CUBE) {  // the single-call launcher's own acceptance test, on this member's floats (model_is_leap reads h_f: an isotropic cube inertia)
    if (!engine_build(m)->accepts(m)) {  // (generation 3: checked above)
      jh_set_error("%s: member %d: the leap kernel does not accept this image (dimensions, table sizes, or h_f: the cube's inertia must be isotropic)", who, b);
      return JH_ERR_UNSUPPORTED;
    }
  }
  if (m->kind == JH_TASK_FR3_PICK) {  // likewise: the build this image selects (arm_pairs) must accept it; jh_model_is_fr3 reads h_f for the finger slides
    if (!engine_build(m)->accepts(m)) {
      jh_set_error("%s: member %d: the %s build of the cooperative arm kernel does not accept this image (dimensions, pair lists, or h_f: the finger slides must be antiparallel)", who, b, engine_build(m)->name);
      return JH_ERR_UNSUPPORTED;
    }
  }
  return JH_OK;
}

static int model_set_upload(jh_model_set* s, int b, const jh_model* m) {
  if (s->nf) JH_HIP(hipMemcpy(s->d_images + (size_t)b * s->stride, m->d_f, 4 * s->nf, hipMemcpyDeviceToDevice));  // (synchronous: not for the plan loop)
  s->hf[b] = m->h_f; s->hi[b] = m->h_i;
  return JH_OK;
}

static int model_set_create(const char* who, const jh_model* const* models, int B, jh_model_set** out, bool fr3) {
  JH_REQUIRE(models && out, "%s: null pointer", who);
  JH_REQUIRE(B >= 1, "%s: B must be at least 1 (B=%d)", who, B);
  JH_REQUIRE(B <= 65535, "%s: B = %d exceeds the 65535 problems of a launch (the grid's second dimension)", who, B);
  for (int b = 0; b < B; b++) if (int rc = model_set_member(who, models[0], models[b], b, fr3)) return rc;
  const jh_model* m0 = models[0];
  JH_HIP(hipSetDevice(m0->device));
  jh_model_set* s = new jh_model_set();
  s->B = B; s->nf = m0->nf; s->stride = (m0->nf + 63) / 64 * 64; s->d_images = nullptr; s->m0 = m0; s->hf.resize(B); s->hi.resize(B); s->d_i_plain = nullptr; s->tables = false;
  if (s->stride == 0) s->stride = 64;
  hipError_t e = hipMalloc(&s->d_images, 4 * s->stride * (size_t)B);
  if (e == hipSuccess) e = hipMemset(s->d_images, 0, 4 * s->stride * (size_t)B);  // (the padding between the images is never read; zero all the same)
  int rc = JH_OK;
  if (e != hipSuccess) { jh_set_error("%s: device allocation failed: %s", who, hipGetErrorString(e)); rc = JH_ERR_HIP; }
  if (rc == JH_OK && hipMalloc(&s->d_i_plain, 4 * (m0->ni ? m0->ni : 1)) != hipSuccess) { jh_set_error("%s: device allocation failed", who); rc = JH_ERR_HIP; }
  for (int b = 0; b < B && rc == JH_OK; b++) rc = model_set_upload(s, b, models[b]);
  if (rc == JH_OK) rc = model_set_tables(s, true);
  if (rc != JH_OK) { if (s->d_images) (void)hipFree(s->d_images); if (s->d_i_plain) (void)hipFree(s->d_i_plain); delete s; return rc; }
  *out = s;
  return JH_OK;
}

extern "C" int jh_model_set_create(const jh_model* const* models, int B, jh_model_set** out) { return model_set_create("model_set_create", models, B, out, false); }

// A set of fr3_pick models (include/judo_amd.h): the same record and the same checks, member by member, for the family the generic constructor refuses; the entries that
// carry a phase plan it.
extern "C" int jh_fr3_model_set_create(const jh_model* const* models, int B, jh_model_set** out) { return model_set_create("fr3_model_set_create", models, B, out, true); }

extern "C" int jh_model_set_update(jh_model_set* s, int b, const jh_model* model) {
  JH_REQUIRE(s && model, "model_set_update: null pointer");
  JH_REQUIRE(b >= 0 && b < s->B, "model_set_update: member %d of a set of %d", b, s->B);
  // (a new member 0 is held to the old one, which the others were held to; it then leads the set.  An fr3 set takes fr3_pick members alone and no other set takes one.)
  if (int rc = model_set_member("model_set_update", s->m0, model, b, s->m0->kind == JH_TASK_FR3_PICK)) return rc;
  JH_HIP(hipSetDevice(s->m0->device));
  if (int rc = model_set_upload(s, b, model)) return rc;
  if (b == 0) s->m0 = model;
  return model_set_tables(s, b == 0);
}

extern "C" int jh_model_set_info(const jh_model_set* s, int* out) {
  JH_REQUIRE(s && out, "model_set_info: null pointer");
  int differ = 0;
  for (int b = 1; b < s->B; b++) differ += s->hf[b].size() != s->hf[0].size() || memcmp(s->hf[b].data(), s->hf[0].data(), 4 * s->hf[0].size()) != 0;
  out[0] = s->B; out[1] = (int)s->nf; out[2] = (int)s->stride; out[3] = differ;
  return JH_OK;
}

// The set's member 0 and its members, for jh_plants.hip: jh_plants_advance checks the kind and the dimensions in front of its first enqueue (jh_internal.h).
const jh_model* jh_model_set_member0(const jh_model_set* s) { return s->m0; }
int jh_model_set_members(const jh_model_set* s) { return s->B; }

extern "C" void jh_model_set_destroy(jh_model_set* s) {
  if (!s) return;
  if (s->d_images) (void)hipFree(s->d_images);
  if (s->d_i_plain) (void)hipFree(s->d_i_plain);
  delete s;
}

extern "C" int jh_model_set_pair_tables(const jh_model_set* s) {
  JH_REQUIRE(s != nullptr, "model_set_pair_tables: null pointer");
  return s->tables && s->hi[0].size() > (size_t)HI_PT && s->hi[0][HI_PT] > 0 ? 1 : 0;
}

extern "C" int jh_plan_step_batch_models(const jh_model_set* set, void* blk_dev, const void* blk_host, size_t blk_bytes, size_t blk_stride_bytes, int o_nominal, int o_sigma, int o_tp, int o_lohi,
                                         const float* noise, int ldn, size_t noise_stride_floats, const float* W, int N, int H, int K, float* costs, float* trace, int mode, float lambda,
                                         int k, int tie_high, int E, int row_floats, int colmajor, float* scratch, float* out, size_t out_stride_floats, void* out_host_mark,
                                         void* const* timing, void* stream) {
  JH_REQUIRE(set != nullptr, "plan_step_batch_models: null pointer");
  return plan_step_batch(JH_BATCH_STEP("plan_step_batch_models", set->m0, set->d_images, (long long)set->stride, set->tables ? set->m0->d_i : set->d_i_plain, set->B));
}

// jh_plan_step_batch_phases on a set of fr3_pick models (include/judo_amd.h): the same code path with the set's images and stride; the int section is member 0's own.
extern "C" int jh_plan_step_batch_phases_models(const jh_model_set* set, int B, void* blk_dev, const void* blk_host, size_t blk_bytes, size_t blk_stride_bytes, int o_nominal, int o_sigma, int o_tp,
                                                int o_lohi, int o_phase, const float* noise, int ldn, size_t noise_stride_floats, const float* W, int N, int H, int K, float* costs, float* trace,
                                                int mode, float lambda, int k, int tie_high, int E, int row_floats, int colmajor, float* scratch, float* out, size_t out_stride_floats,
                                                void* out_host_mark, void* const* timing, void* stream) {
  const char* who = "plan_step_batch_phases_models";
  JH_REQUIRE(set != nullptr, "%s: null pointer", who);
  if (set->m0->kind != JH_TASK_FR3_PICK) { jh_set_error("%s: a phase word per problem is fr3_pick's alone; jh_plan_step_batch_models plans this set", who); return JH_ERR_UNSUPPORTED; }
  JH_REQUIRE(B == set->B, "%s: B = %d problems for a set of %d members: problem b runs on member b", who, B, set->B);
  JH_REQUIRE(o_phase >= 0, "%s: negative block offset (o_phase=%d)", who, o_phase);
  jh_batch_step r = JH_BATCH_STEP(who, set->m0, set->d_images, (long long)set->stride, set->m0->d_i, B);
  r.o_phase = o_phase;
  return plan_step_batch(r);
}
#undef JH_BATCH_STEP

// ---- plan steps on the plants of a model set (include/judo_amd.h): ONE launcher behind the twelve entries, with three degrees of freedom ----
//  - the kind, what the rollout launch's y axis means.  Ensemble: the M members -- every member rolls out the same N candidates from the same block (block and noise
//    strides 0) on its own image into its own row of member_costs, and the tail aggregates the M rows into `costs` (the mean of the `worst` largest) before it updates.
//    With `weights` set the tail is the plant-weighted one (the tail mean under the weights, which travel in the kernel arguments); the rollout launch is the same call.
//    Randomised: G blocks of Nb = N / G rollouts, block g on plant plant_of_block[g] -- block stride 0, noise and cost strides Nb (block g's columns of the one noise
//    matrix, its slice of `costs`), and the plant axis (jh_internal.h) with the rollout-index stride Nb, so that only global rollout 0 drops its noise, and the table, which
//    travels in the kernel arguments; the tail is the plain one on the N costs.
//  - the controller axis (`fleet`), blockIdx.z of the rollout launch: B controllers, each with its own block, noise, costs, output record and `worst` or table row
//    (entry c * G + g), the strides of jh_plan_step_batch between them; a set of M members is shared by all controllers (image stride 0 on that axis), a set of B * M holds
//    controller b's plants at b * M ...  The tail is then the batched one on (tail workgroups, B) with the two-level ticket and one completion word.  Without the axis the
//    tails are the single call's (k_update_tail, k_update_tail_ensemble): not B = 1 of the batched ones.
//    With `o_risk` set, an ensemble's controllers each carry a risk record in their block (the tail word, 0.0 for `worst`, then M weights; the B records are checked on
//    the host) and the batched tail is the one that reads them: the measure per controller and per plan step, where B x M weights would not fit in the kernel arguments.
//  - the phase, fr3_pick's alone (the entries that take one refuse every other family): none, and fr3_pick is refused; `phase` 0..3, one controller's, which travels in the
//    launch record to every member's or block's workgroups; or `o_phase`, the float offset of every controller's phase word in its block (the B words are checked on the host).
// Always two launches (the closed-form models' one-launch form would roll a candidate out on one member per workgroup); no trace buffer, no knots_out.  Every check stands
// in front of the first enqueue.
struct jh_set_step {
  const char* who; const jh_model_set* set;
  void* blk_dev; const void* blk_host; jh_block_shape shape; const float *noise, *W;  // the block (blk_dev == blk_host: read in place, as jh_plan_step), its shape, noise and spline weights
  float* costs; int mode; float lambda; int k, tie_high;                              // the update
  float *scratch, *out; void* out_host_mark; void* const* timing; void* stream;
  const char* fr3_hint = "";                                                          // what a non-phase entry names behind its refusal of fr3_pick
  bool randomized = false;
  float* member_costs = nullptr; const int* worst = nullptr;                          // ensemble: (B x) M x N costs; one `worst`, or B with a controller axis
  const float* weights = nullptr; float tail = 0.f;                                   // ensemble, set: the plant-weighted risk measure (HOST, M) stands where `worst` does
  const unsigned char* plant_of_block = nullptr; int G = 0;                           // randomised: the (B x) G table
  bool fleet = false; int B = 1, M = 0; size_t out_stride_floats = 0;                 // the controller axis (its block and noise strides are the shape's)
  int phase = -1, o_phase = -1;
  int o_risk = -1;                                                                    // ensemble with a controller axis: the float offset of every controller's risk record in its block
};

// The B risk records of jh_plan_step_ensemble_batch_risk, on the host, before anything is enqueued (as phase_words reads the phases): the record's place in the block --
// inside blk_bytes, which the upload copies, and clear of the five sections and the phase word --, then every controller's tail word and, where that is not zero, weights.
static int risk_records(const char* who, const jh_model* m, int B, int M, const void* blk_host, const jh_block_shape& d, int o_phase, int o_risk) {
  const long long lo = o_risk, hi = (long long)o_risk + 1 + M;
  JH_REQUIRE(sizeof(float) * (size_t)hi <= d.bytes, "%s: o_risk = %d: a risk record of 1 + M = %d floats ends outside a block of %zu bytes", who, o_risk, 1 + M, d.bytes);
  const int KU = d.K * m->nu;
  const struct { const char* name; long long at, n; } parts[] = {{"x0", 0, m->nq + m->nv}, {"nominal", d.o_nominal, KU}, {"sigma", d.o_sigma, KU}, {"task params", d.o_tp, m->ntaskparam},
                                                                 {"bounds", d.o_lohi, 2 * m->nu}, {"phase word", o_phase, o_phase >= 0 ? 1 : 0}};
  for (const auto& p : parts)
    JH_REQUIRE(p.n <= 0 || hi <= p.at || p.at + p.n <= lo, "%s: o_risk = %d: the risk record [%lld, %lld) overlaps the block's %s [%lld, %lld)", who, o_risk, lo, hi, p.name, p.at, p.at + p.n);
  for (int b = 0; b < B; b++) {
    const float* rec = reinterpret_cast<const float*>(static_cast<const char*>(blk_host) + (size_t)b * d.stride_bytes) + o_risk;
    const float tail = rec[0];
    JH_REQUIRE(tail >= 0.f && tail <= 1.f, "%s: controller %d: the tail word of its risk record is %g, neither 0 (the `worst` measure) nor in (0, 1]", who, b, (double)tail);  // (false for NaN)
    if (tail == 0.f) continue;
    bool positive = false;
    for (int i = 0; i < M; i++) {
      JH_REQUIRE(std::isfinite(rec[1 + i]) && rec[1 + i] >= 0.f, "%s: controller %d: weights[%d] = %g is negative or not finite", who, b, i, (double)rec[1 + i]);
      positive = positive || rec[1 + i] > 0.f;
    }
    JH_REQUIRE(positive, "%s: controller %d: weights are all zero (M = %d): at least one plant needs a positive weight", who, b, M);
  }
  return JH_OK;
}

static int plan_step_set(const jh_set_step& r) {
  const char* who = r.who;
  const jh_block_shape& d = r.shape;
#define JH_SET_PTR(p) JH_REQUIRE(r.p != nullptr, "%s: " #p " is a null pointer", who)
  JH_SET_PTR(set); JH_SET_PTR(blk_dev); JH_SET_PTR(blk_host); JH_SET_PTR(noise); JH_SET_PTR(W);
  if (r.randomized) JH_SET_PTR(plant_of_block); else { JH_SET_PTR(member_costs); if (!r.weights) JH_SET_PTR(worst); }
  JH_SET_PTR(costs); JH_SET_PTR(scratch); JH_SET_PTR(out);
#undef JH_SET_PTR
  const jh_model_set* set = r.set;
  const jh_model* m = set->m0;
  const int N = d.N, H = d.H, K = d.K, G = r.G, B = r.B, M = r.fleet ? r.M : set->B;
  if (r.fleet) {
    JH_REQUIRE(B >= 1 && B <= JH_MAX_ENSEMBLE_FLEET, "%s: B = %d outside [1, JH_MAX_ENSEMBLE_FLEET = %d]", who, B, JH_MAX_ENSEMBLE_FLEET);
    JH_REQUIRE(M >= 1 && M <= JH_MAX_ENSEMBLE, "%s: M = %d outside [1, JH_MAX_ENSEMBLE = %d]", who, M, JH_MAX_ENSEMBLE);
  } else JH_REQUIRE(M <= JH_MAX_ENSEMBLE, "%s: a set of %d members exceeds JH_MAX_ENSEMBLE = %d", who, M, JH_MAX_ENSEMBLE);
  if (r.randomized) JH_REQUIRE(G >= 1 && G <= JH_MAX_PLANT_BLOCKS, "%s: G = %d outside [1, JH_MAX_PLANT_BLOCKS = %d]", who, G, JH_MAX_PLANT_BLOCKS);
  if (r.randomized && r.fleet)
    JH_REQUIRE(B * G <= JH_MAX_FLEET_PLANT_BLOCKS, "%s: B * G = %d * %d = %d exceeds JH_MAX_FLEET_PLANT_BLOCKS = %d (the bytes of the table in the kernel arguments)", who, B, G, B * G,
               JH_MAX_FLEET_PLANT_BLOCKS);
  if (r.fleet) JH_REQUIRE(set->B == M || set->B == B * M, "%s: a set of %d members is neither the M = %d plants every controller shares nor the B * M = %d plants of B = %d controllers", who, set->B, M, B * M, B);
  jh_upd::EnsembleWeights weights;  // (read here: the caller's array is free when the call returns)
  if (r.weights) { if (int rc = jh_ensemble_weights_check(who, r.weights, M, r.tail, &weights)) return rc; }
  if (!r.randomized && !r.fleet && !r.weights) JH_REQUIRE(r.worst[0] >= 1 && r.worst[0] <= M, "%s: worst = %d outside [1, M = %d]", who, r.worst[0], M);
  if (!r.randomized && r.fleet) for (int b = 0; b < B; b++) JH_REQUIRE(r.worst[b] >= 1 && r.worst[b] <= M, "%s: controller %d: worst = %d outside [1, M = %d]", who, b, r.worst[b], M);
  const bool phased = r.phase >= 0 || r.o_phase >= 0;
  if (m->kind == JH_TASK_FR3_PICK && !phased) { jh_set_error("%s: fr3_pick has no batched plan step (its phase is chosen per problem on the host) behind this entry: %s", who, r.fr3_hint); return JH_ERR_UNSUPPORTED; }
  JH_REQUIRE(!phased || K <= 8, "%s: the cooperative arm kernel keeps at most 8 knots per actuator in registers (K=%d)", who, K);
  if (m->kind == JH_TASK_LEAP_CUBE && m->kernel_gen != 3) { jh_set_error("%s: only kernel generation 3 of the leap family has a batched launch (this model runs %d)", who, m->kernel_gen); return JH_ERR_UNSUPPORTED; }
  if (int rc = check_block_shape(who, m, d)) return rc;
  if (r.randomized) {
    JH_REQUIRE(N % G == 0, "%s: N = %d is no multiple of G = %d (the blocks are N / G rollouts each)", who, N, G);
    for (int e = 0; e < B * G; e++) {
      if (r.fleet) JH_REQUIRE((int)r.plant_of_block[e] < M, "%s: plant_of_block[%d] = %d outside [0, M = %d): controller %d, block %d names no member of the set", who, e, (int)r.plant_of_block[e], M, e / G, e % G);
      else JH_REQUIRE((int)r.plant_of_block[e] < M, "%s: plant_of_block[%d] = %d outside [0, M = %d): block %d names no member of the set", who, e, (int)r.plant_of_block[e], M, e);
    }
  }
  const int KU = K * m->nu;
  if (r.fleet) JH_REQUIRE(r.out_stride_floats >= 2 * (size_t)KU, "%s: out_stride_floats = %zu is smaller than an output record (nominal | sigma = %zu floats)", who, r.out_stride_floats, 2 * (size_t)KU);
  JH_REQUIRE(m->plan_step_launches != 1, "%s: one launch is forced (jh_model_set_plan_step_launches) but %s plan step is two launches", who, r.randomized ? "the randomised" : "the ensemble's");
  const long long rollouts = (long long)B * (r.randomized ? 1 : M) * N;
  JH_REQUIRE(rollouts <= 0x7fffffffll, "%s: %s = %lld rollouts exceed one launch", who, !r.fleet ? "M * N" : r.randomized ? "B * N" : "B * M * N", rollouts);
  const jh_engine_build* eb = engine_build(m);
  if (!(eb && eb->rollout_cost_batch)) { jh_set_error("%s: no batched kernel for this model", who); return JH_ERR_UNSUPPORTED; }
  if (r.o_phase >= 0) { if (int rc = phase_words(who, "controller", B, r.blk_host, d.bytes, d.stride_bytes, r.o_phase)) return rc; }
  const bool risk = r.fleet && !r.randomized && r.o_risk >= 0;
  if (risk) { if (int rc = risk_records(who, m, B, M, r.blk_host, d, r.o_phase, r.o_risk)) return rc; }
  const float* b = (const float*)r.blk_dev;
  jh_upd::TailArgs a;  // (controller 0's record; the tail's own checks before anything is enqueued: mode, lambda, k)
  if (int rc = jh_update_tail_args(who, r.costs, nullptr, b + d.o_nominal, r.noise, d.ldn, b + d.o_sigma, b + d.o_lohi, N, 0, K, m->nu, r.mode, r.lambda, r.k, r.tie_high, 0, nullptr, 0, 0, r.scratch,
                                   r.out, r.out + KU, nullptr, nullptr, &a)) return rc;
  // the y axis of the rollout launch: Y problems of Nb rollouts, whose costs lie Nb and whose noise columns noise_y apart; the plant axis maps a problem to its image
  const int Y = r.randomized ? G : M, Nb = r.randomized ? N / G : N;
  const long long noise_y = r.randomized ? Nb : 0;
  float* rollout_costs = r.randomized ? r.costs : r.member_costs;
  jh_plant_axis plants;
  if (r.randomized) { plants.n_stride = Nb; for (int e = 0; e < B * G; e++) jh_plant_set(plants, e, r.plant_of_block[e]); }
  // ... and the z axis, the controllers (B = 1 and every stride 0 without it)
  const long long blk_c = (long long)(d.stride_bytes / sizeof(float)), noise_c = (long long)d.noise_stride_floats, image_c = (!r.fleet || set->B == M) ? 0ll : (long long)M * (long long)set->stride;
  hipStream_t st = (hipStream_t)r.stream;
  if (int rc = step_begin(r.blk_dev, r.blk_host, (size_t)(B - 1) * d.stride_bytes + d.bytes, r.timing, r.stream)) return rc;
  const jh_step_mark mk = step_mark(r.out_host_mark, r.out);
  if (!r.fleet) { a.done_flag = mk.flag; a.done_value = mk.expect; }  // (with a controller axis the word is the batch ticket's)
  // the rollout launch's record: problem (c, y)'s costs lie (c * Y + y) * Nb behind rollout_costs, the block and the noise are the controller's
  const jh_rollout_args ra = {b, b + d.o_nominal, r.noise, d.ldn, b + d.o_sigma, r.W, b + d.o_lohi, b + d.o_tp, 0, Nb, 0, H, K, rollout_costs, nullptr, nullptr};
  jh_rollout_batch rb = {set->d_images, (long long)set->stride, set->tables ? m->d_i : set->d_i_plain, Y, 0, noise_y, B, blk_c, noise_c, image_c};
  rb.plants = plants; rb.o_phase = r.o_phase; rb.phase = r.phase;
  int rc = eb->rollout_cost_batch(m, ra, rb, st);
  if (rc == JH_OK && r.timing) JH_HIP(hipEventRecord((hipEvent_t)r.timing[1], st));
  if (rc == JH_OK && r.weights) rc = jh_update_tail_ensemble_weighted_launch(a, jh_upd::EnsembleWeightedArgs{r.member_costs, r.costs, M, r.tail, (long long)N, weights}, st);
  else if (rc == JH_OK && !r.fleet) rc = r.randomized ? jh_update_tail_launch(a, st) : jh_update_tail_ensemble_launch(a, jh_upd::EnsembleArgs{r.member_costs, r.costs, M, r.worst[0], (long long)N}, st);
  if (rc == JH_OK && r.fleet) {
    jh_upd::BatchArgs s;  // the tail's axis: the controllers
    s.B = B; s.blk = blk_c; s.noise = noise_c; s.costs = N; s.trace = 0; s.scratch = (long long)jh_update_fused_scratch_floats(N, K, m->nu); s.out = (long long)r.out_stride_floats;
    s.counter = reinterpret_cast<unsigned*>(r.scratch) + 1; s.done_flag = mk.flag; s.done_value = mk.expect;
    jh_upd::EnsembleBatchArgs e;
    e.member_costs = r.member_costs; e.costs = r.costs; e.M = M; e.stride = (long long)N;
    for (int i = 0; i < JH_MAX_ENSEMBLE_FLEET; i++) e.worst[i] = (unsigned char)(!r.randomized && i < B ? r.worst[i] : 1);
    if (risk) {
      jh_upd::EnsembleRiskBatchArgs q;
      q.member_costs = r.member_costs; q.costs = r.costs; q.M = M; q.stride = (long long)N; q.slab = (long long)M * N; q.ldc = s.costs;
      q.risk = b + r.o_risk; q.risk_stride = blk_c;
      for (int i = 0; i < JH_MAX_ENSEMBLE_FLEET; i++) q.worst[i] = e.worst[i];
      rc = jh_update_tail_ensemble_risk_batch_launch(a, s, q, st);
    } else rc = r.randomized ? jh_update_tail_batch_launch(a, s, st) : jh_update_tail_ensemble_batch_launch(a, s, e, st);
  }
  return step_end(rc, r.out, mk, r.timing, r.stream);
}

// The entries: their own pre-checks, then the record.  (`JH_SET_STEP`: the fields every entry has, in the record's order.)
#define JH_SET_STEP(who, batched, blk_stride, noise_stride)                                                                                                       \
  {who, set, blk_dev, blk_host, {blk_bytes, o_nominal, o_sigma, o_tp, o_lohi, ldn, N, H, K, batched, blk_stride, noise_stride}, noise, W, costs, mode, lambda, k, \
   tie_high, scratch, out, out_host_mark, timing, stream}

extern "C" int jh_plan_step_ensemble(const jh_model_set* set, void* blk_dev, const void* blk_host, size_t blk_bytes, int o_nominal, int o_sigma, int o_tp, int o_lohi, const float* noise, int ldn,
                                     const float* W, int N, int H, int K, float* member_costs, float* costs, int worst, int mode, float lambda, int k, int tie_high, float* scratch, float* out,
                                     void* out_host_mark, void* const* timing, void* stream) {
  jh_set_step r = JH_SET_STEP("plan_step_ensemble", false, 0, 0);
  r.fr3_hint = "jh_plan_step_ensemble_phase takes the arm's phase and plans it against the set's plants; jh_plan_step_randomized_phase spreads one arm's candidates over them";
  r.member_costs = member_costs; r.worst = &worst;
  return plan_step_set(r);
}

// jh_plan_step_ensemble with the plant-weighted risk measure: the same record with the weights and the tail mass, so the rollout launch is the same call and the tail
// launch the weighted one.
extern "C" int jh_plan_step_ensemble_weighted(const jh_model_set* set, void* blk_dev, const void* blk_host, size_t blk_bytes, int o_nominal, int o_sigma, int o_tp, int o_lohi, const float* noise,
                                              int ldn, const float* W, int N, int H, int K, float* member_costs, float* costs, const float* weights, float tail, int mode, float lambda, int k,
                                              int tie_high, float* scratch, float* out, void* out_host_mark, void* const* timing, void* stream) {
  const char* who = "plan_step_ensemble_weighted";
  JH_REQUIRE(weights != nullptr, "%s: weights is a null pointer", who);
  jh_set_step r = JH_SET_STEP(who, false, 0, 0);
  r.fr3_hint = "jh_plan_step_ensemble_weighted_phase takes the arm's phase and plans it against the set's plants";
  r.member_costs = member_costs; r.weights = weights; r.tail = tail;
  return plan_step_set(r);
}

// jh_plan_step_ensemble for fr3_pick: the same record with the arm's phase, which the fr3 kernel's members take from the launch record.
extern "C" int jh_plan_step_ensemble_phase(const jh_model_set* set, void* blk_dev, const void* blk_host, size_t blk_bytes, int o_nominal, int o_sigma, int o_tp, int o_lohi, const float* noise,
                                           int ldn, const float* W, int phase, int N, int H, int K, float* member_costs, float* costs, int worst, int mode, float lambda, int k, int tie_high,
                                           float* scratch, float* out, void* out_host_mark, void* const* timing, void* stream) {
  const char* who = "plan_step_ensemble_phase";
  JH_REQUIRE(set != nullptr, "%s: set is a null pointer", who);
  if (set->m0->kind != JH_TASK_FR3_PICK) { jh_set_error("%s: a phase is fr3_pick's alone; jh_plan_step_ensemble plans this set", who); return JH_ERR_UNSUPPORTED; }
  JH_REQUIRE(phase >= 0 && phase <= 3, "%s: phase = %d is not 0, 1, 2 or 3 (LIFT, MOVE, PLACE, HOMING)", who, phase);
  jh_set_step r = JH_SET_STEP(who, false, 0, 0);
  r.member_costs = member_costs; r.worst = &worst; r.phase = phase;
  return plan_step_set(r);
}

// jh_plan_step_ensemble_phase with the plant-weighted risk measure.
extern "C" int jh_plan_step_ensemble_weighted_phase(const jh_model_set* set, void* blk_dev, const void* blk_host, size_t blk_bytes, int o_nominal, int o_sigma, int o_tp, int o_lohi,
                                                    const float* noise, int ldn, const float* W, int phase, int N, int H, int K, float* member_costs, float* costs, const float* weights,
                                                    float tail, int mode, float lambda, int k, int tie_high, float* scratch, float* out, void* out_host_mark, void* const* timing,
                                                    void* stream) {
  const char* who = "plan_step_ensemble_weighted_phase";
  JH_REQUIRE(set != nullptr, "%s: set is a null pointer", who);
  if (set->m0->kind != JH_TASK_FR3_PICK) { jh_set_error("%s: a phase is fr3_pick's alone; jh_plan_step_ensemble_weighted plans this set", who); return JH_ERR_UNSUPPORTED; }
  JH_REQUIRE(phase >= 0 && phase <= 3, "%s: phase = %d is not 0, 1, 2 or 3 (LIFT, MOVE, PLACE, HOMING)", who, phase);
  JH_REQUIRE(weights != nullptr, "%s: weights is a null pointer", who);
  jh_set_step r = JH_SET_STEP(who, false, 0, 0);
  r.member_costs = member_costs; r.weights = weights; r.tail = tail; r.phase = phase;
  return plan_step_set(r);
}

extern "C" int jh_plan_step_randomized(const jh_model_set* set, void* blk_dev, const void* blk_host, size_t blk_bytes, int o_nominal, int o_sigma, int o_tp, int o_lohi, const float* noise, int ldn,
                                       const float* W, int N, int H, int K, const unsigned char* plant_of_block, int G, float* costs, int mode, float lambda, int k, int tie_high, float* scratch,
                                       float* out, void* out_host_mark, void* const* timing, void* stream) {
  jh_set_step r = JH_SET_STEP("plan_step_randomized", false, 0, 0);
  r.fr3_hint = "jh_plan_step_randomized_phase takes the arm's phase";
  r.randomized = true; r.plant_of_block = plant_of_block; r.G = G;
  return plan_step_set(r);
}

// jh_plan_step_randomized for fr3_pick: the same record with the arm's phase, which the fr3 kernel's blocks take from the launch record.
extern "C" int jh_plan_step_randomized_phase(const jh_model_set* set, void* blk_dev, const void* blk_host, size_t blk_bytes, int o_nominal, int o_sigma, int o_tp, int o_lohi, const float* noise,
                                             int ldn, const float* W, int phase, int N, int H, int K, const unsigned char* plant_of_block, int G, float* costs, int mode, float lambda, int k,
                                             int tie_high, float* scratch, float* out, void* out_host_mark, void* const* timing, void* stream) {
  const char* who = "plan_step_randomized_phase";
  JH_REQUIRE(set != nullptr, "%s: set is a null pointer", who);
  if (set->m0->kind != JH_TASK_FR3_PICK) { jh_set_error("%s: a phase is fr3_pick's alone; jh_plan_step_randomized plans this set", who); return JH_ERR_UNSUPPORTED; }
  JH_REQUIRE(phase >= 0 && phase <= 3, "%s: phase = %d is not 0, 1, 2 or 3 (LIFT, MOVE, PLACE, HOMING)", who, phase);
  jh_set_step r = JH_SET_STEP(who, false, 0, 0);
  r.randomized = true; r.plant_of_block = plant_of_block; r.G = G; r.phase = phase;
  return plan_step_set(r);
}

extern "C" int jh_plan_step_ensemble_batch(const jh_model_set* set, int B, int M, void* blk_dev, const void* blk_host, size_t blk_bytes, size_t blk_stride_bytes, int o_nominal, int o_sigma, int o_tp,
                                           int o_lohi, const float* noise, int ldn, size_t noise_stride_floats, const float* W, int N, int H, int K, float* member_costs, float* costs,
                                           const int* worst, int mode, float lambda, int k, int tie_high, float* scratch, float* out, size_t out_stride_floats, void* out_host_mark,
                                           void* const* timing, void* stream) {
  jh_set_step r = JH_SET_STEP("plan_step_ensemble_batch", true, blk_stride_bytes, noise_stride_floats);
  r.fr3_hint = "jh_plan_step_ensemble_batch_phases takes a phase word per controller; jh_plan_step_batch_phases_models plans B arms on B plants";
  r.member_costs = member_costs; r.worst = worst;
  r.fleet = true; r.B = B; r.M = M; r.out_stride_floats = out_stride_floats;
  return plan_step_set(r);
}

// jh_plan_step_ensemble_batch for fr3_pick: the same record with a phase word in every controller's block.
extern "C" int jh_plan_step_ensemble_batch_phases(const jh_model_set* set, int B, int M, void* blk_dev, const void* blk_host, size_t blk_bytes, size_t blk_stride_bytes, int o_nominal, int o_sigma,
                                                  int o_tp, int o_lohi, int o_phase, const float* noise, int ldn, size_t noise_stride_floats, const float* W, int N, int H, int K, float* member_costs,
                                                  float* costs, const int* worst, int mode, float lambda, int k, int tie_high, float* scratch, float* out, size_t out_stride_floats,
                                                  void* out_host_mark, void* const* timing, void* stream) {
  const char* who = "plan_step_ensemble_batch_phases";
  JH_REQUIRE(set != nullptr, "%s: set is a null pointer", who);
  if (set->m0->kind != JH_TASK_FR3_PICK) { jh_set_error("%s: a phase word per controller is fr3_pick's alone; jh_plan_step_ensemble_batch plans this set", who); return JH_ERR_UNSUPPORTED; }
  JH_REQUIRE(o_phase >= 0, "%s: negative block offset (o_phase=%d)", who, o_phase);
  jh_set_step r = JH_SET_STEP(who, true, blk_stride_bytes, noise_stride_floats);
  r.member_costs = member_costs; r.worst = worst; r.o_phase = o_phase;
  r.fleet = true; r.B = B; r.M = M; r.out_stride_floats = out_stride_floats;
  return plan_step_set(r);
}

// jh_plan_step_ensemble_batch with a risk record in every controller's block (include/judo_amd.h): the same record with `o_risk`, so the rollout launch is the same call
// and the tail launch the one that reads the records.
extern "C" int jh_plan_step_ensemble_batch_risk(const jh_model_set* set, int B, int M, void* blk_dev, const void* blk_host, size_t blk_bytes, size_t blk_stride_bytes, int o_nominal, int o_sigma,
                                                int o_tp, int o_lohi, int o_risk, const float* noise, int ldn, size_t noise_stride_floats, const float* W, int N, int H, int K, float* member_costs,
                                                float* costs, const int* worst, int mode, float lambda, int k, int tie_high, float* scratch, float* out, size_t out_stride_floats,
                                                void* out_host_mark, void* const* timing, void* stream) {
  const char* who = "plan_step_ensemble_batch_risk";
  JH_REQUIRE(o_risk >= 0, "%s: negative block offset (o_risk=%d)", who, o_risk);
  jh_set_step r = JH_SET_STEP(who, true, blk_stride_bytes, noise_stride_floats);
  r.fr3_hint = "jh_plan_step_ensemble_batch_phases_risk takes a phase word per controller as well";
  r.member_costs = member_costs; r.worst = worst; r.o_risk = o_risk;
  r.fleet = true; r.B = B; r.M = M; r.out_stride_floats = out_stride_floats;
  return plan_step_set(r);
}

// jh_plan_step_ensemble_batch_phases with a risk record in every controller's block.
extern "C" int jh_plan_step_ensemble_batch_phases_risk(const jh_model_set* set, int B, int M, void* blk_dev, const void* blk_host, size_t blk_bytes, size_t blk_stride_bytes, int o_nominal,
                                                       int o_sigma, int o_tp, int o_lohi, int o_phase, int o_risk, const float* noise, int ldn, size_t noise_stride_floats, const float* W, int N,
                                                       int H, int K, float* member_costs, float* costs, const int* worst, int mode, float lambda, int k, int tie_high, float* scratch, float* out,
                                                       size_t out_stride_floats, void* out_host_mark, void* const* timing, void* stream) {
  const char* who = "plan_step_ensemble_batch_phases_risk";
  JH_REQUIRE(set != nullptr, "%s: set is a null pointer", who);
  if (set->m0->kind != JH_TASK_FR3_PICK) { jh_set_error("%s: a phase word per controller is fr3_pick's alone; jh_plan_step_ensemble_batch_risk plans this set", who); return JH_ERR_UNSUPPORTED; }
  JH_REQUIRE(o_phase >= 0, "%s: negative block offset (o_phase=%d)", who, o_phase);
  JH_REQUIRE(o_risk >= 0, "%s: negative block offset (o_risk=%d)", who, o_risk);
  jh_set_step r = JH_SET_STEP(who, true, blk_stride_bytes, noise_stride_floats);
  r.member_costs = member_costs; r.worst = worst; r.o_phase = o_phase; r.o_risk = o_risk;
  r.fleet = true; r.B = B; r.M = M; r.out_stride_floats = out_stride_floats;
  return plan_step_set(r);
}

extern "C" int jh_plan_step_randomized_batch(const jh_model_set* set, int B, int M, void* blk_dev, const void* blk_host, size_t blk_bytes, size_t blk_stride_bytes, int o_nominal, int o_sigma,
                                             int o_tp, int o_lohi, const float* noise, int ldn, size_t noise_stride_floats, const float* W, int N, int H, int K,
                                             const unsigned char* plant_of_block, int G, float* costs, int mode, float lambda, int k, int tie_high, float* scratch, float* out,
                                             size_t out_stride_floats, void* out_host_mark, void* const* timing, void* stream) {
  jh_set_step r = JH_SET_STEP("plan_step_randomized_batch", true, blk_stride_bytes, noise_stride_floats);
  r.fr3_hint = "jh_plan_step_randomized_batch_phases takes a phase word per controller; jh_plan_step_randomized_phase plans one arm over the set's plants and jh_plan_step_batch_phases_models B arms on B plants";
  r.randomized = true; r.plant_of_block = plant_of_block; r.G = G;
  r.fleet = true; r.B = B; r.M = M; r.out_stride_floats = out_stride_floats;
  return plan_step_set(r);
}

// jh_plan_step_randomized_batch for fr3_pick: the same record with a phase word in every controller's block.
extern "C" int jh_plan_step_randomized_batch_phases(const jh_model_set* set, int B, int M, void* blk_dev, const void* blk_host, size_t blk_bytes, size_t blk_stride_bytes, int o_nominal, int o_sigma,
                                                    int o_tp, int o_lohi, int o_phase, const float* noise, int ldn, size_t noise_stride_floats, const float* W, int N, int H, int K,
                                                    const unsigned char* plant_of_block, int G, float* costs, int mode, float lambda, int k, int tie_high, float* scratch, float* out,
                                                    size_t out_stride_floats, void* out_host_mark, void* const* timing, void* stream) {
  const char* who = "plan_step_randomized_batch_phases";
  JH_REQUIRE(set != nullptr, "%s: set is a null pointer", who);
  if (set->m0->kind != JH_TASK_FR3_PICK) { jh_set_error("%s: a phase word per controller is fr3_pick's alone; jh_plan_step_randomized_batch plans this set", who); return JH_ERR_UNSUPPORTED; }
  JH_REQUIRE(o_phase >= 0, "%s: negative block offset (o_phase=%d)", who, o_phase);
  jh_set_step r = JH_SET_STEP(who, true, blk_stride_bytes, noise_stride_floats);
  r.randomized = true; r.plant_of_block = plant_of_block; r.G = G; r.o_phase = o_phase;
  r.fleet = true; r.B = B; r.M = M; r.out_stride_floats = out_stride_floats;
  return plan_step_set(r);
}
#undef JH_SET_STEP

// The update alone for B problems whose costs are given (the materialise path of a fleet: the Spot policy rollout, judo_amd/fleet.py): jh_plan_step_batch's last stage --
// k_update_tail_batch with the two-level ticket -- and its completion mark, without an upload or a rollout kernel in front.
extern "C" int jh_update_fused_batch(int B, const float* costs, const float* blk, size_t blk_stride_floats, int o_nominal, int o_sigma, int o_lohi, const float* noise, int ldn,
                                     size_t noise_stride_floats, int N, int K, int nu, int mode, float lambda, int k, int tie_high, int E, const float* trace, int row_floats,
                                     int colmajor, float* scratch, float* out, size_t out_stride_floats, void* out_host_mark, void* stream) {
  JH_REQUIRE(costs && blk && noise && scratch && out, "update_fused_batch: null pointer");
  JH_REQUIRE(B >= 1, "update_fused_batch: B must be at least 1 (B=%d)", B);
  JH_REQUIRE(B <= 65535, "update_fused_batch: B = %d exceeds the 65535 problems of a launch (the grid's second dimension)", B);
  JH_REQUIRE(N > 0 && K > 0 && nu > 0 && K * nu <= JH_MAX_KNOT_DIM, "update_fused_batch: N, K, nu must be positive and K*nu <= %d (N=%d K=%d nu=%d)", JH_MAX_KNOT_DIM, N, K, nu);
  JH_REQUIRE(o_nominal >= 0 && o_sigma >= 0 && o_lohi >= 0, "update_fused_batch: negative block offset");
  const int KU = K * nu;
  const size_t need = (size_t)std::max(std::max(o_nominal + KU, o_sigma + KU), o_lohi + 2 * nu);
  JH_REQUIRE(blk_stride_floats >= need, "update_fused_batch: blk_stride_floats = %zu is smaller than a block (nominal | sigma | bounds at the given offsets end at %zu floats)", blk_stride_floats, need);
  JH_REQUIRE(ldn >= N && noise_stride_floats >= (size_t)KU * (size_t)ldn, "update_fused_batch: ldn (%d) < N (%d), or noise_stride_floats = %zu is smaller than a problem's noise (K*nu*ldn = %zu)", ldn, N,
             noise_stride_floats, (size_t)KU * (size_t)ldn);
  const int E_t = trace ? E : 0;
  JH_REQUIRE(E_t >= 0 && E_t <= JH_MAX_ELITES && (E_t == 0 || row_floats >= 1), "update_fused_batch: bad trace arguments (E=%d row_floats=%d)", E, row_floats);
  const size_t rec = 2 * (size_t)KU + (size_t)E_t * (2 + (size_t)(E_t > 0 ? row_floats : 0));
  JH_REQUIRE(out_stride_floats >= rec, "update_fused_batch: out_stride_floats = %zu is smaller than an output record (nominal | sigma | E trace records = %zu floats)", out_stride_floats, rec);
  const jh_step_mark mk = step_mark(out_host_mark, out);
  jh_upd::TailArgs a;
  if (int rc = jh_update_tail_args("update_fused_batch", costs, nullptr, blk + o_nominal, noise, ldn, blk + o_sigma, blk + o_lohi, N, 0, K, nu, mode, lambda, k, tie_high, E_t, trace, row_floats,
                                   colmajor, scratch, out, out + KU, E_t > 0 ? out + 2 * KU : nullptr, nullptr, &a)) return rc;
  jh_upd::BatchArgs s;
  s.B = B; s.blk = (long long)blk_stride_floats; s.noise = (long long)noise_stride_floats; s.costs = N; s.trace = (long long)N * row_floats;
  s.scratch = (long long)jh_update_fused_scratch_floats(N, K, nu); s.out = (long long)out_stride_floats;
  s.counter = reinterpret_cast<unsigned*>(scratch) + 1; s.done_flag = mk.flag; s.done_value = mk.expect;
  return step_end(jh_update_tail_batch_launch(a, s, (hipStream_t)stream), out, mk, nullptr, stream);
}

// The same iteration when the rollouts are sharded over G ranks: launch -> all-gather -> merge.  The tail writes this rank's record; jh_plan_merge
// finishes the update on every rank (jh_shard_merge: identical nominal everywhere, no broadcast) into the same output block jh_plan_step fills and sets the same
// completion mark.
extern "C" int jh_plan_step_shard(const jh_model* m, void* blk_dev, const void* blk_host, size_t blk_bytes, int o_nominal, int o_sigma, int o_tp, int o_lohi, const float* noise,
                                  int ldn, const float* W, int phase, int N, int n_offset, int H, int K, float* costs, float* knots_out, float* trace, int mode, float lambda, int k,
                                  int tie_high, int E, int row_floats, int colmajor, float* scratch, float* rec_out, void* const* timing /* 3 events, or NULL */, void* stream) {
  JH_REQUIRE(rec_out, "plan_step_shard: null pointer");
  return plan_step("plan_step_shard", m, blk_dev, blk_host, blk_bytes, o_nominal, o_sigma, o_tp, o_lohi, noise, ldn, W, phase, N, n_offset, H, K, costs, knots_out, trace, mode,
                   lambda, k, tie_high, E, row_floats, colmajor, scratch, nullptr, nullptr, rec_out, timing, stream);
}

extern "C" int jh_plan_merge(const float* recs, int G, int K, int nu, int mode, float lambda, int k, int tie_high, int E, int row_floats, float* out, void* out_host_mark,
                             void* timing_done /* event of jh_event_create recorded behind the merge, or NULL */, void* stream) {
  JH_REQUIRE(recs && out, "plan_merge: null pointer");
  const int KU = K * nu;
  int rc = jh_shard_merge(recs, G, K, nu, mode, lambda, k, tie_high, E, row_floats, out, out + KU, E > 0 ? out + 2 * KU : nullptr, stream);
  if (rc == JH_OK && timing_done) JH_HIP(hipEventRecord((hipEvent_t)timing_done, (hipStream_t)stream));
  if (rc == JH_OK) rc = jh_download_begin(out_host_mark, out, 0, stream);
  return rc;
}

// Timing events for callers that bracket kernels on the launch stream without torch (bench.py's roofline leg: the rollout kernel's duration inside a jh_plan_step call)
extern "C" int jh_event_create(void** out) { JH_REQUIRE(out, "event_create: null pointer"); hipEvent_t e; JH_HIP(hipEventCreate(&e)); *out = e; return JH_OK; }
extern "C" void jh_event_destroy(void* ev) { if (ev) (void)hipEventDestroy((hipEvent_t)ev); }
extern "C" int jh_event_record(void* ev, void* stream) { JH_REQUIRE(ev, "event_record: null pointer"); JH_HIP(hipEventRecord((hipEvent_t)ev, (hipStream_t)stream)); return JH_OK; }
extern "C" int jh_stream_wait_event(void* stream, void* ev) {  // device-side: work enqueued on `stream` after this call waits for `ev` (recorded on another stream)
  JH_REQUIRE(ev, "stream_wait_event: null pointer");
  JH_HIP(hipStreamWaitEvent((hipStream_t)stream, (hipEvent_t)ev, 0));
  return JH_OK;
}
extern "C" int jh_event_elapsed_ms(void* a, void* b, float* ms) {  // waits for b
  JH_REQUIRE(a && b && ms, "event_elapsed_ms: null pointer");
  JH_HIP(hipEventSynchronize((hipEvent_t)b));
  JH_HIP(hipEventElapsedTime(ms, (hipEvent_t)a, (hipEvent_t)b));
  return JH_OK;
}

extern "C" int jh_rollout_materialize(const jh_model* m, const float* x0, int x0_batched, const float* controls, int N, int H, float* states,
                                      float* sensors, void* stream) {
  JH_REQUIRE(m && x0 && controls, "rollout_materialize: null pointer");
  JH_REQUIRE(states || sensors, "rollout_materialize: both outputs are null");
  JH_REQUIRE(N > 0 && H > 0, "rollout_materialize: N and H must be positive (N=%d H=%d)", N, H);
  hipStream_t st = (hipStream_t)stream;
  if (const jh_engine_build* eb = engine_build(m)) return eb->materialize(m, x0, x0_batched, controls, N, H, states, sensors, st);
  if (!g_xcheck.rollout_materialize) { jh_set_error("rollout_materialize: no kernel for this model / generation in this library"); return JH_ERR_UNSUPPORTED; }
  return g_xcheck.rollout_materialize(m, m->kernel_gen, x0, x0_batched, controls, N, H, states, sensors, stream);
}

// jh_rollout_materialize on the plants of a model set (include/judo_amd.h): G blocks of n rollouts in ONE launch on grid (workgroups of a block, G), block g on image
// plant_of_block[g].  The table travels in the kernel arguments (jh_plant_axis); the int section is the set's one copy, by the rule the plan steps on a set use.  Every
// check stands in front of the first enqueue.  Both entries' body: `fr3_entry` is jh_fr3_rollout_materialize_plants, which takes an fr3_pick set and no other; the
// general entry takes every other family's.
static int materialize_plants_entry(const char* who, bool fr3_entry, const jh_model_set* set, const int* plant_of_block, int G, int n, const float* x0, int x0_batched, const float* controls,
                                    int controls_shared, int H, float* states, float* sensors, void* stream) {
#define JH_MP_PTR(p) JH_REQUIRE((p) != nullptr, "%s: " #p " is a null pointer", who)
  JH_MP_PTR(set); JH_MP_PTR(plant_of_block); JH_MP_PTR(x0); JH_MP_PTR(controls);
#undef JH_MP_PTR
  JH_REQUIRE(states || sensors, "%s: states and sensors are both null: nothing to compute", who);
  const jh_model* m = set->m0;
  const int M = set->B;
  if (!fr3_entry && m->kind == JH_TASK_FR3_PICK) {
    // (the wording is pinned by the tests of this entry; what serves the set stands behind it)
    jh_set_error("%s: an fr3_pick set: behind this entry the cooperative arm kernel has no materialise launch on plants yet; "
                 "jh_fr3_rollout_materialize_plants rolls an fr3_pick set out, and jh_rollout_materialize on a member's own handle rolls one plant out", who);
    return JH_ERR_UNSUPPORTED;
  }
  if (fr3_entry && m->kind != JH_TASK_FR3_PICK) {
    jh_set_error("%s: not an fr3_pick set: this entry is the cooperative arm kernel's; jh_rollout_materialize_plants rolls every other family's set out", who);
    return JH_ERR_UNSUPPORTED;
  }
  JH_REQUIRE(M <= JH_MAX_ENSEMBLE, "%s: a set of %d members exceeds JH_MAX_ENSEMBLE = %d", who, M, JH_MAX_ENSEMBLE);
  JH_REQUIRE(G >= 1 && G <= JH_MAX_FLEET_PLANT_BLOCKS, "%s: G = %d outside [1, JH_MAX_FLEET_PLANT_BLOCKS = %d] (the bytes of the table in the kernel arguments)", who, G, JH_MAX_FLEET_PLANT_BLOCKS);
  JH_REQUIRE(n >= 1, "%s: n = %d must be at least 1", who, n);
  JH_REQUIRE(H >= 1, "%s: H = %d must be at least 1", who, H);
  for (int g = 0; g < G; g++) JH_REQUIRE(plant_of_block[g] >= 0 && plant_of_block[g] < M, "%s: plant_of_block[%d] = %d outside [0, M = %d): block %d names no member of the set", who, g, plant_of_block[g], M, g);
  JH_REQUIRE((long long)G * n <= 0x7fffffffll, "%s: G * n = %d * %d rollouts exceed one launch", who, G, n);
  const jh_engine_build* eb = engine_build(m);
  if (!(eb && eb->materialize_plants)) { jh_set_error("%s: no materialise kernel on plants for this model / kernel generation", who); return JH_ERR_UNSUPPORTED; }
  jh_rollout_batch rb = {set->d_images, (long long)set->stride, set->tables ? m->d_i : set->d_i_plain, G, 0, 0};
  for (int g = 0; g < G; g++) jh_plant_set(rb.plants, g, plant_of_block[g]);
  return eb->materialize_plants(m, rb, x0, x0_batched, controls, controls_shared, n, H, states, sensors, (hipStream_t)stream);
}

extern "C" int jh_rollout_materialize_plants(const jh_model_set* set, const int* plant_of_block, int G, int n, const float* x0, int x0_batched, const float* controls, int controls_shared,
                                             int H, float* states, float* sensors, void* stream) {
  return materialize_plants_entry("rollout_materialize_plants", false, set, plant_of_block, G, n, x0, x0_batched, controls, controls_shared, H, states, sensors, stream);
}

// The same call for an fr3_pick set (include/judo_amd.h): the cooperative arm kernel's materialise launch on plants, behind an entry of its own as every fr3 form is.  The
// argument checks are the one function above; the int section is the model's own (fr3 sets share it word for word).
extern "C" int jh_fr3_rollout_materialize_plants(const jh_model_set* set, const int* plant_of_block, int G, int n, const float* x0, int x0_batched, const float* controls, int controls_shared,
                                                 int H, float* states, float* sensors, void* stream) {
  return materialize_plants_entry("fr3_rollout_materialize_plants", true, set, plant_of_block, G, n, x0, x0_batched, controls, controls_shared, H, states, sensors, stream);
}

extern "C" int jh_task_reward(const jh_model* m, const float* states, const float* sensors, const float* controls, const float* tp, int phase, int N,
                              int H, float* rewards, void* stream) {
  JH_REQUIRE(m && states && tp && rewards, "task_reward: null pointer");
  JH_REQUIRE(N > 0 && H > 0, "task_reward: N and H must be positive");
  hipStream_t st = (hipStream_t)stream;
  if (m->kind == JH_TASK_CARTPOLE || m->kind == JH_TASK_CYLINDER_PUSH) {
    JH_REQUIRE(m->kind != JH_TASK_CARTPOLE || controls, "task_reward: cartpole needs controls");
    return jh_simple_reward(m, states, controls, tp, N, H, rewards, st);
  }
  return jh_engine_reward(m, states, sensors, controls, tp, phase, N, H, rewards, st);
}
