// jh_plants.hip -- the plant side of the closed loop (include/judo_amd.h fixes the arithmetic, judo_amd/simulation.py restates it): B device-resident plants advance S
// physics steps on the splines their controllers planned, in ONE call.
//   k_plant_controls   controls[b, step0 + s, u] = sum_k W[b, s, k] * knots[b, k, u], k ascending, then clipped: plant b's spline at plant b's own clock, W host-built
//   the materialise launch on plants (jh_rollout_materialize_plants / jh_fr3_rollout_materialize_plants): B blocks of one row, block b on plant truth[b], from x[b]
//   k_plant_reports    what a robot reports of the segment -- state + sigma * noise where the step and the column are reported, NaN elsewhere -- and the carry x[b] <-
//                      states[b, S - 1], the exact state
// A translation unit of its own: no existing code object changes.  Every product and sum is rounded on its own.  The library is compiled with -ffp-contract=fast, which
// fuses across statements whatever `#pragma clang fp contract(off)` says; the two kernels' bodies therefore have strict floating-point semantics, as k_plant_residuals
// has.  No floating-point compare stands in them (this compiler cannot lower a strict one for gfx950): the clip compares the values' order-preserving integer keys.
#include "jh_internal.h"

namespace {
constexpr int kThreads = 256;

// The step phases of the B plants of a launch, by value: (steps taken before the segment) mod `every`.
struct PlantPhases {
  int phase[JH_MAX_FLEET_PLANT_BLOCKS];
};

// An unsigned key with key(a) < key(b) exactly when a < b as floats (-0.0 below +0.0; NaNs at the two ends).
__device__ __forceinline__ unsigned order_key(float v) {
  const unsigned b = __float_as_uint(v);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

__global__ __launch_bounds__(kThreads) void k_plant_controls(const float* __restrict__ W, const float* __restrict__ knots, size_t knot_stride, const float* __restrict__ lohi,
                                                             int S, int K, int nu, int step0, int ld_steps, float* __restrict__ controls) {
#pragma clang fp exceptions(strict)
  const int i = blockIdx.x * kThreads + threadIdx.x;  // s * nu + u
  if (i >= S * nu) return;
  const int b = blockIdx.y, s = i / nu, u = i % nu;
  const float* w = W + ((size_t)b * S + s) * K;
  const float* kn = knots + (size_t)b * knot_stride + u;
  float acc = w[0] * kn[0];
  for (int k = 1; k < K; k++) {
    const float p = w[k] * kn[(size_t)k * nu];
    acc = acc + p;
  }
  if (lohi != nullptr) {  // min(hi, max(lo, acc)) on the keys; a NaN passes through
    const float lo = lohi[u], hi = lohi[nu + u];
    const bool nan = (__float_as_uint(acc) & 0x7fffffffu) > 0x7f800000u;
    if (!nan && order_key(acc) < order_key(lo)) acc = lo;
    if (!nan && order_key(acc) > order_key(hi)) acc = hi;
  }
  controls[((size_t)b * ld_steps + step0 + s) * nu + u] = acc;
}

// One entry of a report: row-major (S, n) of plant b, element i.
__device__ __forceinline__ bool reported_at(int phase, int every, int s, const unsigned char* mask, int j) {
  return (phase + s + 1) % every == 0 && (mask == nullptr || mask[j] != 0);
}

__global__ __launch_bounds__(kThreads) void k_plant_reports(const float* __restrict__ states, const float* __restrict__ sensors, int S, int nx, int ns, PlantPhases ph, int every,
                                                            const float* __restrict__ noise, const float* __restrict__ sigma, const unsigned char* __restrict__ mask,
                                                            float* __restrict__ reports, const float* __restrict__ noise_sens, const float* __restrict__ sigma_sens,
                                                            const unsigned char* __restrict__ mask_sens, float* __restrict__ reports_sens, float* __restrict__ x) {
#pragma clang fp exceptions(strict)
  const int i = blockIdx.x * kThreads + threadIdx.x;
  const int b = blockIdx.y, phase = ph.phase[b];
  const float not_reported = __uint_as_float(0x7fc00000u);
  if (reports != nullptr && i < S * nx) {
    const size_t at = (size_t)b * S * nx + i;
    const int s = i / nx, j = i % nx;
    float v = not_reported;
    if (reported_at(phase, every, s, mask, j)) {
      v = states[at];
      if (sigma != nullptr && noise != nullptr) {
        const float p = sigma[j] * noise[at];
        v = v + p;
      }
    }
    reports[at] = v;
  }
  if (reports_sens != nullptr && i < S * ns) {
    const size_t at = (size_t)b * S * ns + i;
    const int s = i / ns, j = i % ns;
    float v = not_reported;
    if (reported_at(phase, every, s, mask_sens, j)) {
      v = sensors[at];
      if (sigma_sens != nullptr && noise_sens != nullptr) {
        const float p = sigma_sens[j] * noise_sens[at];
        v = v + p;
      }
    }
    reports_sens[at] = v;
  }
  if (i < nx) x[(size_t)b * nx + i] = states[((size_t)b * S + (S - 1)) * nx + i];  // the carry: the exact state, never the noisy one
}

int check_controls(const char* who, const float* W, const float* knots, size_t knot_stride, int B, int S, int K, int nu, int step0, int ld_steps, const float* controls) {
  JH_REQUIRE(W != nullptr, "%s: W is a null pointer", who);
  JH_REQUIRE(knots != nullptr, "%s: knots is a null pointer", who);
  JH_REQUIRE(controls != nullptr, "%s: controls is a null pointer", who);
  JH_REQUIRE(B >= 1 && B <= JH_MAX_FLEET_PLANT_BLOCKS, "%s: B = %d outside [1, JH_MAX_FLEET_PLANT_BLOCKS = %d]", who, B, JH_MAX_FLEET_PLANT_BLOCKS);
  JH_REQUIRE(S >= 1, "%s: S = %d must be at least 1", who, S);
  JH_REQUIRE(K >= 1, "%s: K = %d must be at least 1", who, K);
  JH_REQUIRE(nu >= 1, "%s: nu = %d must be at least 1", who, nu);
  JH_REQUIRE((long long)K * nu <= JH_MAX_KNOT_DIM, "%s: K * nu = %d * %d exceeds JH_MAX_KNOT_DIM = %d", who, K, nu, JH_MAX_KNOT_DIM);
  JH_REQUIRE(B == 1 || knot_stride >= (size_t)K * nu, "%s: knot_stride = %zu is smaller than a plant's K * nu = %d knots", who, knot_stride, K * nu);
  JH_REQUIRE(step0 >= 0, "%s: step0 = %d is negative", who, step0);
  JH_REQUIRE((long long)ld_steps >= (long long)step0 + S, "%s: ld_steps (%d) < step0 + S (%d + %d)", who, ld_steps, step0, S);
  JH_REQUIRE((long long)S * nu <= 0x7fffffffll, "%s: S * nu = %d * %d beyond one launch", who, S, nu);
  return JH_OK;
}

void launch_controls(const float* W, const float* knots, size_t knot_stride, const float* lohi, int B, int S, int K, int nu, int step0, int ld_steps, float* controls, hipStream_t st) {
  hipLaunchKernelGGL(k_plant_controls, dim3((unsigned)((S * nu + kThreads - 1) / kThreads), (unsigned)B), dim3(kThreads), 0, st, W, knots, knot_stride, lohi, S, K, nu, step0,
                     ld_steps, controls);
}

// The report arguments of both entries; fills the phases.
int check_reports(const char* who, int B, int S, int nx, int ns, const int* count, int every, const float* states, const float* sensors, const float* reports_sens, const float* x,
                  PlantPhases& ph) {
  JH_REQUIRE(states != nullptr, "%s: states is a null pointer", who);
  JH_REQUIRE(x != nullptr, "%s: x is a null pointer", who);
  JH_REQUIRE(count != nullptr, "%s: count is a null pointer", who);
  JH_REQUIRE(B >= 1 && B <= JH_MAX_FLEET_PLANT_BLOCKS, "%s: B = %d outside [1, JH_MAX_FLEET_PLANT_BLOCKS = %d]", who, B, JH_MAX_FLEET_PLANT_BLOCKS);
  JH_REQUIRE(S >= 1, "%s: S = %d must be at least 1", who, S);
  JH_REQUIRE(nx >= 1, "%s: nx = %d must be at least 1", who, nx);
  JH_REQUIRE(ns >= 0, "%s: ns = %d is negative", who, ns);
  JH_REQUIRE(every >= 1, "%s: every = %d must be at least 1", who, every);
  JH_REQUIRE(reports_sens == nullptr || (ns >= 1 && sensors != nullptr), "%s: reports_sens is given with ns = %d and sensors %s: there are no sensor rows to report", who, ns,
             sensors ? "given" : "a null pointer");
  JH_REQUIRE((long long)S * nx <= 0x7fffffffll && (long long)S * ns <= 0x7fffffffll, "%s: S * nx = %d * %d or S * ns = %d * %d beyond one launch", who, S, nx, S, ns);
  for (int b = 0; b < B; b++) {
    JH_REQUIRE(count[b] >= 0, "%s: count[%d] = %d is negative: plant %d has taken no such number of steps", who, b, count[b], b);
    ph.phase[b] = count[b] % every;
  }
  return JH_OK;
}

void launch_reports(const float* states, const float* sensors, int B, int S, int nx, int ns, const PlantPhases& ph, int every, const float* noise, const float* sigma,
                    const unsigned char* mask, float* reports, const float* noise_sens, const float* sigma_sens, const unsigned char* mask_sens, float* reports_sens, float* x,
                    hipStream_t st) {
  const int n = S * (nx > ns ? nx : ns);
  hipLaunchKernelGGL(k_plant_reports, dim3((unsigned)((n + kThreads - 1) / kThreads), (unsigned)B), dim3(kThreads), 0, st, states, sensors, S, nx, ns, ph, every, noise, sigma, mask,
                     reports, noise_sens, sigma_sens, mask_sens, reports_sens, x);
}
}  // namespace

extern "C" int jh_plant_controls(const float* W, const float* knots, size_t knot_stride, const float* ctrl_lo_hi, int B, int S, int K, int nu, int step0, int ld_steps,
                                 float* controls, void* stream) {
  if (int rc = check_controls("plant_controls", W, knots, knot_stride, B, S, K, nu, step0, ld_steps, controls)) return rc;
  launch_controls(W, knots, knot_stride, ctrl_lo_hi, B, S, K, nu, step0, ld_steps, controls, (hipStream_t)stream);
  JH_HIP(hipGetLastError());
  return JH_OK;
}

extern "C" int jh_plant_reports(const float* states, const float* sensors, int B, int S, int nx, int ns, const int* count, int every, const float* noise, const float* sigma,
                                const unsigned char* column_mask, float* reports, const float* noise_sens, const float* sigma_sens, const unsigned char* column_mask_sens,
                                float* reports_sens, float* x, void* stream) {
  PlantPhases ph{};
  if (int rc = check_reports("plant_reports", B, S, nx, ns, count, every, states, sensors, reports_sens, x, ph)) return rc;
  launch_reports(states, sensors, B, S, nx, ns, ph, every, noise, sigma, column_mask, reports, noise_sens, sigma_sens, column_mask_sens, reports_sens, x, (hipStream_t)stream);
  JH_HIP(hipGetLastError());
  return JH_OK;
}

extern "C" int jh_plants_advance(const jh_model_set* set, const int* truth, int B, float* x, const float* W, const float* knots, size_t knot_stride, int K,
                                 const float* ctrl_lo_hi, int step0, int S, float* controls, float* states, float* sensors, const int* count, int every, const float* noise,
                                 const float* sigma, const unsigned char* column_mask, float* reports, const float* noise_sens, const float* sigma_sens,
                                 const unsigned char* column_mask_sens, float* reports_sens, void* stream) {
  const char* who = "plants_advance";
  JH_REQUIRE(set != nullptr, "%s: set is a null pointer", who);
  JH_REQUIRE(truth != nullptr, "%s: truth is a null pointer", who);
  const jh_model* m = jh_model_set_member0(set);
  const int M = jh_model_set_members(set), nx = m->nq + m->nv;
  const bool closed_form = m->kind == JH_TASK_CARTPOLE || m->kind == JH_TASK_CYLINDER_PUSH;
  if (!closed_form && !((m->kind == JH_TASK_LEAP_CUBE || m->kind == JH_TASK_FR3_PICK) && m->kernel_gen == 3)) {
    jh_set_error("%s: no materialise kernel on plants for this model / kernel generation (kind %d, generation %d)", who, m->kind, m->kernel_gen);
    return JH_ERR_UNSUPPORTED;
  }
  JH_REQUIRE(M <= JH_MAX_ENSEMBLE, "%s: a set of %d members exceeds JH_MAX_ENSEMBLE = %d", who, M, JH_MAX_ENSEMBLE);
  JH_REQUIRE(step0 >= 0 && step0 < S, "%s: step0 = %d outside [0, S = %d): the call fills the controls of steps step0 .. S - 1", who, step0, S);
  if (int rc = check_controls(who, W, knots, knot_stride, B, S - step0, K, m->nu, step0, S, controls)) return rc;
  PlantPhases ph{};
  if (int rc = check_reports(who, B, S, nx, m->ns, count, every, states, sensors, reports_sens, x, ph)) return rc;
  for (int b = 0; b < B; b++)
    JH_REQUIRE(truth[b] >= 0 && truth[b] < M, "%s: truth[%d] = %d outside [0, M = %d): plant %d names no member of the set", who, b, truth[b], M, b);
  hipStream_t st = (hipStream_t)stream;
  launch_controls(W, knots, knot_stride, ctrl_lo_hi, B, S - step0, K, m->nu, step0, S, controls, st);
  JH_HIP(hipGetLastError());
  // B blocks of one row, block b on plant truth[b], x0 a row per plant, controls a row per plant, H = S
  const int rc = m->kind == JH_TASK_FR3_PICK ? jh_fr3_rollout_materialize_plants(set, truth, B, 1, x, 1, controls, 0, S, states, sensors, stream)
                                             : jh_rollout_materialize_plants(set, truth, B, 1, x, 1, controls, 0, S, states, sensors, stream);
  if (rc != JH_OK) return rc;
  launch_reports(states, sensors, B, S, nx, m->ns, ph, every, noise, sigma, column_mask, reports, noise_sens, sigma_sens, column_mask_sens, reports_sens, x, st);
  JH_HIP(hipGetLastError());
  return JH_OK;
}
