// jh_reports.hip -- jh_plant_residuals_reports: the plants' prediction errors on recorded windows whose observations are a robot's reports (include/judo_amd.h fixes
// the arithmetic, judo_amd/reports.py plant_residuals_reports_host restates it).  An observed entry that is NaN was not reported and is no evidence: its term is +0.0
// and neither the prediction nor the weight under it is read into the sum.  The reported entries are scored as jh_plant_residuals scores them (jh_reward.hip), sensor
// readings continue the step's sum behind the state, and the window-row a (plant, window) pair reads is m * plant_stride + w * window_stride, which serves the
// plant-major launch of a GpuModelSet and the window-major one of jh_policy_rollout_plants alike.
// A translation unit of its own: the code object of jh_reward.hip, k_plant_residuals with it, is the parent's.
// One wave per (plant, window) pair, lane h holds step h of the window; four waves to a workgroup.  Every product and sum is rounded on its own.  The library is
// compiled with -ffp-contract=fast, which fuses across statements whatever `#pragma clang fp contract(off)` says; the kernel's body therefore has strict floating-point
// semantics, whose operations the compiler neither fuses nor reorders.  Every test is on the bits (this compiler cannot lower a strict floating-point compare for gfx950).
#include "jh_internal.h"

namespace {
constexpr int kIdWaves = 4;  // waves (pairs) of a workgroup

struct QuatAdr {
  int adr[JH_MAX_ID_QUATS];
};

__device__ __forceinline__ bool is_nan_bits(float v) { return (__float_as_uint(v) & 0x7fffffffu) > 0x7f800000u; }

__global__ __launch_bounds__(kIdWaves * 64) void k_plant_residuals_reports(const float* __restrict__ pred, const float* __restrict__ obs, const float* __restrict__ weight,
                                                                            const float* __restrict__ pred_sens, const float* __restrict__ obs_sens,
                                                                            const float* __restrict__ weight_sens, QuatAdr qa, int nquat, int ns, size_t plant_stride,
                                                                            size_t window_stride, long long pairs, int W, int H, int nx, float* __restrict__ err, int ld) {
#pragma clang fp exceptions(strict)
  const long long pair = (long long)blockIdx.x * kIdWaves + (threadIdx.x >> 6);  // m * W + w, uniform over the wave
  if (pair >= pairs) return;
  const int h = threadIdx.x & 63;
  const long long m = pair / W, w = pair % W;
  float s = 0.f;  // (+0.0 in the lanes behind the window's last step: the padding of the halving below)
  if (h < H) {
    const size_t row = (size_t)m * plant_stride + (size_t)w * window_stride;  // the window-row of the prediction, states and sensors alike
    const float* p = pred + (row * H + h) * nx;
    const float* o = obs + ((size_t)w * H + h) * nx;
    bool flip[JH_MAX_ID_QUATS];
#pragma unroll
    for (int i = 0; i < JH_MAX_ID_QUATS; i++) {
      flip[i] = false;
      if (i < nquat) {
        const int a = qa.adr[i];
        float dot = p[a] * o[a];
        dot = dot + p[a + 1] * o[a + 1];
        dot = dot + p[a + 2] * o[a + 2];
        dot = dot + p[a + 3] * o[a + 3];
        // dot < 0 on the bits: negative, neither -0.0 nor NaN -- an unreported coordinate makes dot NaN, hence no flip
        flip[i] = __float_as_uint(dot) > 0x80000000u && __float_as_uint(dot) <= 0xff800000u;
      }
    }
    for (int d = 0; d < nx; d++) {
      float od = o[d];
      float t = 0.f;  // not reported: no evidence
      if (!is_nan_bits(od)) {
#pragma unroll
        for (int i = 0; i < JH_MAX_ID_QUATS; i++)
          if (i < nquat && flip[i] && d >= qa.adr[i] && d < qa.adr[i] + 4) od = -od;
        const float e = p[d] - od;
        t = (weight[d] * e) * e;
      }
      s = d == 0 ? t : s + t;
    }
    if (ns > 0) {
      const float* ps = pred_sens + (row * H + h) * ns;
      const float* os = obs_sens + ((size_t)w * H + h) * ns;
      for (int d = 0; d < ns; d++) {
        const float od = os[d];
        float t = 0.f;
        if (!is_nan_bits(od)) {
          const float e = ps[d] - od;
          t = (weight_sens[d] * e) * e;
        }
        s = s + t;
      }
    }
  }
  for (int off = 32; off >= 1; off >>= 1) s = s + __shfl_down(s, off);  // v[i] += v[i + off]: the lanes below `off` hold the live half
  if (h == 0) err[m * ld + w] = s;
}
}  // namespace

extern "C" int jh_plant_residuals_reports(const float* pred, const float* obs, const float* weight, const int* quat_adr, int nquat, const float* pred_sens, const float* obs_sens,
                                          const float* weight_sens, int ns, size_t plant_stride, size_t window_stride, int M, int W, int H, int nx, int nq, float* err, int ld,
                                          void* stream) {
  JH_REQUIRE(pred != nullptr, "plant_residuals_reports: pred is a null pointer");
  JH_REQUIRE(obs != nullptr, "plant_residuals_reports: obs is a null pointer");
  JH_REQUIRE(weight != nullptr, "plant_residuals_reports: weight is a null pointer");
  JH_REQUIRE(err != nullptr, "plant_residuals_reports: err is a null pointer");
  JH_REQUIRE(M >= 1 && M <= JH_MAX_ENSEMBLE, "plant_residuals_reports: M = %d outside [1, JH_MAX_ENSEMBLE = %d]", M, JH_MAX_ENSEMBLE);
  JH_REQUIRE(W >= 1, "plant_residuals_reports: W = %d must be at least 1", W);
  JH_REQUIRE(H >= 1 && H <= JH_MAX_ID_HORIZON, "plant_residuals_reports: H = %d outside [1, JH_MAX_ID_HORIZON = %d]", H, JH_MAX_ID_HORIZON);
  JH_REQUIRE(nx >= 1, "plant_residuals_reports: nx = %d must be at least 1", nx);
  JH_REQUIRE(nq >= 0 && nq <= nx, "plant_residuals_reports: nq = %d outside [0, nx = %d]", nq, nx);
  JH_REQUIRE(ld >= W, "plant_residuals_reports: ld (%d) < W (%d)", ld, W);
  JH_REQUIRE(nquat >= 0 && nquat <= JH_MAX_ID_QUATS, "plant_residuals_reports: nquat = %d outside [0, JH_MAX_ID_QUATS = %d]", nquat, JH_MAX_ID_QUATS);
  JH_REQUIRE(nquat == 0 || quat_adr != nullptr, "plant_residuals_reports: quat_adr is a null pointer with nquat = %d", nquat);
  JH_REQUIRE(ns >= 0, "plant_residuals_reports: ns = %d is negative", ns);
  JH_REQUIRE(ns == 0 || pred_sens != nullptr, "plant_residuals_reports: pred_sens is a null pointer with ns = %d", ns);
  JH_REQUIRE(ns == 0 || obs_sens != nullptr, "plant_residuals_reports: obs_sens is a null pointer with ns = %d", ns);
  JH_REQUIRE(ns == 0 || weight_sens != nullptr, "plant_residuals_reports: weight_sens is a null pointer with ns = %d", ns);
  JH_REQUIRE(ns > 0 || pred_sens == nullptr, "plant_residuals_reports: pred_sens is not a null pointer with ns = 0");
  JH_REQUIRE(ns > 0 || obs_sens == nullptr, "plant_residuals_reports: obs_sens is not a null pointer with ns = 0");
  JH_REQUIRE(ns > 0 || weight_sens == nullptr, "plant_residuals_reports: weight_sens is not a null pointer with ns = 0");
  JH_REQUIRE(plant_stride >= 1, "plant_residuals_reports: plant_stride = 0 (window-rows between two plants' predictions of a window; at least 1)");
  JH_REQUIRE(window_stride >= 1, "plant_residuals_reports: window_stride = 0 (window-rows between a plant's predictions of two windows; at least 1)");
  QuatAdr qa{};
  for (int i = 0; i < nquat; i++) {
    const int a = quat_adr[i];
    JH_REQUIRE(a >= 0 && a <= nq - 4, "plant_residuals_reports: quat_adr[%d] = %d: its four coordinates do not lie in [0, nq = %d)", i, a, nq);
    for (int j = 0; j < i; j++)
      JH_REQUIRE(a >= quat_adr[j] + 4 || a + 4 <= quat_adr[j], "plant_residuals_reports: quat_adr[%d] = %d overlaps quat_adr[%d] = %d", i, a, j, quat_adr[j]);
    qa.adr[i] = a;
  }
  const long long pairs = (long long)M * W;  // (kernel indices are 64-bit; the grid's x dimension holds 2^31 - 1 workgroups)
  JH_REQUIRE((pairs + kIdWaves - 1) / kIdWaves <= 0x7fffffffLL, "plant_residuals_reports: M * W = %d * %d beyond the workgroups of one launch", M, W);
  hipLaunchKernelGGL(k_plant_residuals_reports, dim3((unsigned)((pairs + kIdWaves - 1) / kIdWaves)), dim3(kIdWaves * 64), 0, (hipStream_t)stream, pred, obs, weight, pred_sens,
                     obs_sens, weight_sens, qa, nquat, ns, plant_stride, window_stride, pairs, W, H, nx, err, ld);
  JH_HIP(hipGetLastError());
  return JH_OK;
}
