// jh_reward.hip -- Task.reward of the articulated tasks on materialised device arrays (judo/tasks/leap_cube.py:63-88, fr3_pick.py:225-311): one lane per
// rollout walks its H rows; the per-step terms are the ones the fused kernels accumulate (jh_engine_common.h).
#include "jh_engine_common.h"

using namespace jh_eng;

namespace {
constexpr int kBlock = 64;

__global__ __launch_bounds__(kBlock) void k_leap_reward(const float* __restrict__ states, const float* __restrict__ tp, int N, int H, int nx,
                                                        float* __restrict__ rewards) {
  __shared__ float sTp[9];
  if (threadIdx.x < 9) sTp[threadIdx.x] = tp[threadIdx.x];
  __syncthreads();
  const int n = blockIdx.x * kBlock + threadIdx.x;
  if (n >= N) return;
  float acc = 0.f;
  for (int h = 0; h < H; h++) {
    float q[7];
    for (int i = 0; i < 7; i++) q[i] = states[((size_t)n * H + h) * nx + i];
    acc += leap_step_cost(sTp, q);
  }
  rewards[n] = -acc / (float)H;
}

__global__ __launch_bounds__(kBlock) void k_fr3_reward(const float* __restrict__ states, const float* __restrict__ sensors, const float* __restrict__ tp,
                                                       int phase, int N, int H, float* __restrict__ rewards) {
  __shared__ float sTp[22];
  if (threadIdx.x < 22) sTp[threadIdx.x] = tp[threadIdx.x];
  __syncthreads();
  const int n = blockIdx.x * kBlock + threadIdx.x;
  if (n >= N) return;
  float acc = 0.f;
  for (int h = 0; h < H; h++) {
    float x[31], y[14];
    for (int i = 0; i < 31; i++) x[i] = states[((size_t)n * H + h) * 31 + i];
    for (int i = 0; i < 14; i++) y[i] = sensors[((size_t)n * H + h) * 14 + i];
    acc += fr3_step_cost(sTp, phase, x, x + 16, 15, y, H > 1 ? 1.f - (float)h / (float)(H - 1) : 1.f);
  }
  rewards[n] = -acc;
}
}  // namespace

int jh_engine_reward(const jh_model* m, const float* states, const float* sensors, const float* controls, const float* tp, int phase, int N, int H,
                     float* rewards, hipStream_t st) {
  (void)controls;
  int grid = (N + kBlock - 1) / kBlock;
  if (m->kind == JH_TASK_LEAP_CUBE) hipLaunchKernelGGL(k_leap_reward, dim3(grid), dim3(kBlock), 0, st, states, tp, N, H, m->nq + m->nv, rewards);
  else if (m->kind == JH_TASK_FR3_PICK) {
    JH_REQUIRE(sensors != nullptr, "task_reward: fr3_pick needs the sensor array");
    JH_REQUIRE(phase >= 0 && phase <= 3, "task_reward: fr3_pick phase must be 0..3 (got %d)", phase);
    hipLaunchKernelGGL(k_fr3_reward, dim3(grid), dim3(kBlock), 0, st, states, sensors, tp, phase, N, H, rewards);
  } else { jh_set_error("task_reward: unknown articulated task"); return JH_ERR_UNSUPPORTED; }
  JH_HIP(hipGetLastError());
  return JH_OK;
}

// ------------------------------------------------------------------------------------------------ the plants' prediction errors on recorded windows
// (Defined last in the file: the kernel is emitted behind the two above and shifts neither in the code object.)
// jh_plant_residuals scores what a materialise launch on M plants predicted for W recorded windows against what was observed (include/judo_amd.h fixes the arithmetic,
// judo_amd/identify.py plant_residuals_host restates it).  One wave per (plant, window) pair, lane h holds step h of the window; four waves to a workgroup.  Every
// product and sum is rounded on its own.  The library is compiled with -ffp-contract=fast, which fuses across statements whatever `#pragma clang fp contract(off)` says,
// and HIP's __fmul_rn is a plain `*`; the kernel's body therefore has strict floating-point semantics, whose operations the compiler neither fuses nor reorders.
namespace {
constexpr int kIdWaves = 4;  // waves (pairs) of a workgroup

struct QuatAdr {
  int adr[JH_MAX_ID_QUATS];
};

__global__ __launch_bounds__(kIdWaves * 64) void k_plant_residuals(const float* __restrict__ pred, const float* __restrict__ obs, const float* __restrict__ weight,
                                                                    QuatAdr qa, int nquat, long long pairs, int W, int H, int nx, float* __restrict__ err, int ld) {
#pragma clang fp exceptions(strict)
  const long long pair = (long long)blockIdx.x * kIdWaves + (threadIdx.x >> 6);  // m * W + w, uniform over the wave
  if (pair >= pairs) return;
  const int h = threadIdx.x & 63;
  const long long m = pair / W, w = pair % W;
  float s = 0.f;  // (+0.0 in the lanes behind the window's last step: the padding of the halving below)
  if (h < H) {
    const float* p = pred + ((size_t)pair * H + h) * nx;
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
        // dot < 0 on the bits: negative, neither -0.0 nor NaN (this compiler cannot lower a strict floating-point compare for gfx950)
        flip[i] = __float_as_uint(dot) > 0x80000000u && __float_as_uint(dot) <= 0xff800000u;
      }
    }
    for (int d = 0; d < nx; d++) {
      float od = o[d];
#pragma unroll
      for (int i = 0; i < JH_MAX_ID_QUATS; i++)
        if (i < nquat && flip[i] && d >= qa.adr[i] && d < qa.adr[i] + 4) od = -od;
      const float e = p[d] - od;
      const float t = (weight[d] * e) * e;
      s = d == 0 ? t : s + t;
    }
  }
  for (int off = 32; off >= 1; off >>= 1) s = s + __shfl_down(s, off);  // v[i] += v[i + off]: the lanes below `off` hold the live half
  if (h == 0) err[m * ld + w] = s;
}
}  // namespace

extern "C" int jh_plant_residuals(const float* pred, const float* obs, const float* weight, const int* quat_adr, int nquat, int M, int W, int H, int nx, int nq, float* err,
                                  int ld, void* stream) {
  JH_REQUIRE(pred != nullptr, "plant_residuals: pred is a null pointer");
  JH_REQUIRE(obs != nullptr, "plant_residuals: obs is a null pointer");
  JH_REQUIRE(weight != nullptr, "plant_residuals: weight is a null pointer");
  JH_REQUIRE(err != nullptr, "plant_residuals: err is a null pointer");
  JH_REQUIRE(M >= 1 && M <= JH_MAX_ENSEMBLE, "plant_residuals: M = %d outside [1, JH_MAX_ENSEMBLE = %d]", M, JH_MAX_ENSEMBLE);
  JH_REQUIRE(W >= 1, "plant_residuals: W = %d must be at least 1", W);
  JH_REQUIRE(H >= 1 && H <= JH_MAX_ID_HORIZON, "plant_residuals: H = %d outside [1, JH_MAX_ID_HORIZON = %d]", H, JH_MAX_ID_HORIZON);
  JH_REQUIRE(nx >= 1, "plant_residuals: nx = %d must be at least 1", nx);
  JH_REQUIRE(nq >= 0 && nq <= nx, "plant_residuals: nq = %d outside [0, nx = %d]", nq, nx);
  JH_REQUIRE(ld >= W, "plant_residuals: ld (%d) < W (%d)", ld, W);
  JH_REQUIRE(nquat >= 0 && nquat <= JH_MAX_ID_QUATS, "plant_residuals: nquat = %d outside [0, JH_MAX_ID_QUATS = %d]", nquat, JH_MAX_ID_QUATS);
  JH_REQUIRE(nquat == 0 || quat_adr != nullptr, "plant_residuals: quat_adr is a null pointer with nquat = %d", nquat);
  QuatAdr qa{};
  for (int i = 0; i < nquat; i++) {
    const int a = quat_adr[i];
    JH_REQUIRE(a >= 0 && a <= nq - 4, "plant_residuals: quat_adr[%d] = %d: its four coordinates do not lie in [0, nq = %d)", i, a, nq);
    for (int j = 0; j < i; j++)
      JH_REQUIRE(a >= quat_adr[j] + 4 || a + 4 <= quat_adr[j], "plant_residuals: quat_adr[%d] = %d overlaps quat_adr[%d] = %d", i, a, j, quat_adr[j]);
    qa.adr[i] = a;
  }
  const long long pairs = (long long)M * W;  // (kernel indices are 64-bit; the grid's x dimension holds 2^31 - 1 workgroups)
  JH_REQUIRE((pairs + kIdWaves - 1) / kIdWaves <= 0x7fffffffLL, "plant_residuals: M * W = %d * %d beyond the workgroups of one launch", M, W);
  hipLaunchKernelGGL(k_plant_residuals, dim3((unsigned)((pairs + kIdWaves - 1) / kIdWaves)), dim3(kIdWaves * 64), 0, (hipStream_t)stream, pred, obs, weight, qa, nquat, pairs,
                     W, H, nx, err, ld);
  JH_HIP(hipGetLastError());
  return JH_OK;
}
