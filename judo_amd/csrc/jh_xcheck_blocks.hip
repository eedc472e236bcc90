// jh_xcheck_blocks.hip -- TEST BUILD ONLY (libjudo_amd_xcheck.so): the solver's device building blocks of jh_engine_common.h and jh_coop.h, each alone.
//
// The shipped kernels reach these routines only from inside a physics step: a wrong Hessian block or line-search curvature does not move Newton's fixed point, a
// reduction whose lanes disagree in the last bit shows on rare inputs only, and the Cholesky's pivot clamp or the impedance's generic-power branch are reached by almost
// no state of the shipped models.  This file calls one family per launch on n independent cases and writes everything the routine returns, so that
// tests/test_gpu_solver_blocks.py can hold each to an fp64 reference (tests/blocks.py).  The instantiations are the shipped kernels' own; the file is compiled with the
// common flags (the engine files carry their own), so comparisons with a reference are to a tolerance -- the bit claims checked are those between two routines of THIS
// translation unit, and between the lanes of one call.
//
// Scalar families run one case per lane.  Row families run one case per DPP row -- four independent cases per wave, all 64 lanes active (a lane that is switched off
// reads as 0 to its DPP partners: the routines are written for callers at wave-uniform points; n is then a number of LANES and a multiple of 64).  Every case reads
// JH_BLK_IN[family] floats and writes JH_BLK_OUT[family]; the layouts are at the family's code below.
// No loop here depends on data.
#include <hip/hip_runtime.h>

#include "jh_coop.h"

using namespace jh_eng;
using namespace jh_coop;

namespace {

enum { FAM_CONE = 0, FAM_PYRAMID, FAM_CONTACT, FAM_IMPEDANCE, FAM_FRAME, FAM_CHOL3, FAM_CHOL6, FAM_CHOL7, FAM_CHOL4, FAM_ROW, FAM_ARM, FAM_COUNT };
constexpr int JH_BLK_IN[FAM_COUNT] = {16, 16, 16, 8, 4, 36, 36, 36, 16, 20, 64};
constexpr int JH_BLK_OUT[FAM_COUNT] = {24, 24, 24, 1, 9, 44, 44, 44, 24, 28, 18};
constexpr bool JH_BLK_ROWS[FAM_COUNT] = {false, false, false, false, false, false, false, false, false, true, true};

// a second copy of an input that the compiler cannot tell from a new value: the two routines of a bit claim are then compiled each on its own, not merged into one
__device__ __forceinline__ float opaque(float x) { asm volatile("" : "+v"(x)); return x; }

// in: jar[3], jp[3], D[3], Dm, mu, fri, d1 and d2 on entry, cone.
// out: cone_eval's s, f[3], W[6] | cone_top (1 / 0) | cone_below's f[3], W[6] (left untouched where cone_top holds) | cone_dir's d1, d2.
__device__ __forceinline__ void run_cone(const float* c, float* o) {
  const float jar[3] = {c[0], c[1], c[2]}, jp[3] = {c[3], c[4], c[5]}, D[3] = {c[6], c[7], c[8]}, Dm = c[9], mu = c[10], fri = c[11];
  float f[3], W[6];
  o[0] = cone_eval(jar, D, Dm, mu, fri, f, W);
  for (int k = 0; k < 3; k++) o[1 + k] = f[k];
  for (int k = 0; k < 6; k++) o[4 + k] = W[k];
  const float jar2[3] = {opaque(c[0]), opaque(c[1]), opaque(c[2])}, D2[3] = {opaque(c[6]), opaque(c[7]), opaque(c[8])}, Dm2 = opaque(c[9]), mu2 = opaque(c[10]), fri2 = opaque(c[11]);
  ConeZ z;
  const bool top = cone_top(jar2, mu2, fri2, z);
  o[10] = top ? 1.f : 0.f;
  if (!top) {
    float f2[3], W2[6];
    cone_below(jar2, D2, Dm2, mu2, fri2, z, f2, W2);
    for (int k = 0; k < 3; k++) o[11 + k] = f2[k];
    for (int k = 0; k < 6; k++) o[14 + k] = W2[k];
  }
  float d1 = c[12], d2 = c[13];
  cone_dir(jar, jp, D, Dm, mu, fri, &d1, &d2);
  o[20] = d1; o[21] = d2;
}

// in: as run_cone.  out: s, f[3], W[6] of pyramid_eval(jar, D[0], mu) / of contact_eval(cone, jar, D, mu, fri)
__device__ __forceinline__ void run_pyramid(const float* c, float* o, bool contact) {
  const float jar[3] = {c[0], c[1], c[2]}, D[3] = {c[6], c[7], c[8]}, mu = c[10], fri = c[11];
  float f[3], W[6];
  o[0] = contact ? contact_eval((int)c[14], jar, D, mu, fri, f, W) : pyramid_eval(jar, D[0], mu, f, W);
  for (int k = 0; k < 3; k++) o[1 + k] = f[k];
  for (int k = 0; k < 6; k++) o[4 + k] = W[k];
}

// in: packed lower A (N (N + 1) / 2 floats), b[N] at 28.  out: chol_packed<N>'s factor | fwd_packed<N>(b) at 28 | bwd_packed<N> of that at 35.
template <int N>
__device__ __forceinline__ void run_chol(const float* c, float* o) {
  constexpr int T = N * (N + 1) / 2;
  float a[T], v[N];
  for (int k = 0; k < T; k++) a[k] = c[k];
  for (int k = 0; k < N; k++) v[k] = c[28 + k];
  chol_packed<N>(a);
  for (int k = 0; k < T; k++) o[k] = a[k];
  fwd_packed<N>(v, a);
  for (int k = 0; k < N; k++) o[28 + k] = v[k];
  bwd_packed<N>(v, a);
  for (int k = 0; k < N; k++) o[35 + k] = v[k];
}

// in: packed lower A (10), b[4] at 10.  out: chol4's L (10) | inv (4) | fwd4(b) at 14 | bwd4 of that at 18.
__device__ __forceinline__ void run_chol4(const float* c, float* o) {
  float L[10], inv[4], x[4];
  for (int k = 0; k < 10; k++) L[k] = c[k];
  for (int k = 0; k < 4; k++) x[k] = c[10 + k];
  chol4(L, inv);
  for (int k = 0; k < 10; k++) o[k] = L[k];
  for (int k = 0; k < 4; k++) o[10 + k] = inv[k];
  fwd4(L, inv, x);
  for (int k = 0; k < 4; k++) o[14 + k] = x[k];
  bwd4(L, inv, x);
  for (int k = 0; k < 4; k++) o[18 + k] = x[k];
}

// One lane of a DPP row.  in: v | sv[16] at 1 | an int (its bits) at 17.
// out: csum, gsum, qsum4, qsum4_same, row_scatter16(sv), gmin | gor, gmini of the int (bits) | quad_get(v, 0..3) at 8 | row_bcast<0..15>(v) at 12.
__device__ __forceinline__ void run_row(const float* c, float* o, int l) {
  const float v = c[0];
  const int iv = __float_as_int(c[17]);
  float sv[16];
  for (int k = 0; k < 16; k++) sv[k] = c[1 + k];
  o[0] = csum(v); o[1] = gsum(v); o[2] = qsum4(v); o[3] = qsum4_same(v); o[4] = row_scatter16(sv, l); o[5] = gmin(v);
  o[6] = __int_as_float(gor(iv)); o[7] = __int_as_float(gmini(iv));
  o[8] = quad_get(v, 0); o[9] = quad_get(v, 1); o[10] = quad_get(v, 2); o[11] = quad_get(v, 3);
  static_for<16>([&](auto nc) { constexpr int N = decltype(nc)::value; o[12 + N] = row_bcast<N>(v); });
}

// One lane of a DPP row.  in: this lane's R[9] as arm_chol_solve takes it (lane 6 + a: row a of the matrix, lane 15: the right-hand side) | the whole system for
// chol_solve<9>: packed lower A (45) at 9, b[9] at 54.  out: arm_chol_solve's x[9] | chol_solve<9>'s x[9].
__device__ __forceinline__ void run_arm(const float* c, float* o, int l) {
  float R[9], x[9], L[45], y[9];
  for (int k = 0; k < 9; k++) { R[k] = c[k]; x[k] = 0.f; y[k] = c[54 + k]; }
  for (int k = 0; k < 45; k++) L[k] = c[9 + k];
  arm_chol_solve(R, x, l);
  chol_solve<9>(L, y);
  for (int k = 0; k < 9; k++) { o[k] = x[k]; o[9 + k] = y[k]; }
}

template <int FAM>
__global__ __launch_bounds__(64) void k_blocks(const float* __restrict__ in, int n, float* __restrict__ out) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;  // (a row family's n is a multiple of 64: no wave of it loses a lane here)
  const float* c = in + (size_t)i * JH_BLK_IN[FAM];
  float* o = out + (size_t)i * JH_BLK_OUT[FAM];
  const int l = threadIdx.x & 15;
  if constexpr (FAM == FAM_CONE) run_cone(c, o);
  else if constexpr (FAM == FAM_PYRAMID) run_pyramid(c, o, false);
  else if constexpr (FAM == FAM_CONTACT) run_pyramid(c, o, true);
  else if constexpr (FAM == FAM_IMPEDANCE) o[0] = impedance(c, c[5]);
  else if constexpr (FAM == FAM_FRAME) { float fr[9] = {c[0], c[1], c[2], 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}; make_frame(fr); for (int k = 0; k < 9; k++) o[k] = fr[k]; }
  else if constexpr (FAM == FAM_CHOL3) run_chol<3>(c, o);
  else if constexpr (FAM == FAM_CHOL6) run_chol<6>(c, o);
  else if constexpr (FAM == FAM_CHOL7) run_chol<7>(c, o);
  else if constexpr (FAM == FAM_CHOL4) run_chol4(c, o);
  else if constexpr (FAM == FAM_ROW) run_row(c, o, l);
  else run_arm(c, o, l);
}

template <int FAM>
void launch(const float* in, int n, float* out, hipStream_t st) { hipLaunchKernelGGL(k_blocks<FAM>, dim3((n + 63) / 64), dim3(64), 0, st, in, n, out); }

}  // namespace

// family: 0 cone_eval + cone_top / cone_below + cone_dir, 1 pyramid_eval, 2 contact_eval, 3 impedance, 4 make_frame, 5 / 6 / 7 chol_packed + fwd_packed + bwd_packed <3 / 6 / 7>,
// 8 chol4 + fwd4 + bwd4, 9 the row reductions and broadcasts, 10 arm_chol_solve + chol_solve<9>.  `in` (n x in_f) and `out` (n x out_f) are device pointers; in_f and out_f
// are the caller's idea of the family's strides and must be this file's.  Not product interface: bound by tests/blocks.py alone.
extern "C" int jh_xcheck_blocks(int family, const float* in, int in_f, int n, float* out, int out_f, void* stream) {
  JH_REQUIRE(family >= 0 && family < FAM_COUNT, "jh_xcheck_blocks: family %d", family);
  JH_REQUIRE(in && out && n >= 0, "jh_xcheck_blocks: null argument or n < 0");
  JH_REQUIRE(in_f == JH_BLK_IN[family] && out_f == JH_BLK_OUT[family], "jh_xcheck_blocks: family %d has strides %d / %d, not %d / %d", family, JH_BLK_IN[family], JH_BLK_OUT[family], in_f, out_f);
  JH_REQUIRE(!JH_BLK_ROWS[family] || n % 64 == 0, "jh_xcheck_blocks: family %d runs whole waves, n = %d", family, n);
  if (n == 0) return JH_OK;
  hipStream_t st = (hipStream_t)stream;
  switch (family) {
    case FAM_CONE: launch<FAM_CONE>(in, n, out, st); break;
    case FAM_PYRAMID: launch<FAM_PYRAMID>(in, n, out, st); break;
    case FAM_CONTACT: launch<FAM_CONTACT>(in, n, out, st); break;
    case FAM_IMPEDANCE: launch<FAM_IMPEDANCE>(in, n, out, st); break;
    case FAM_FRAME: launch<FAM_FRAME>(in, n, out, st); break;
    case FAM_CHOL3: launch<FAM_CHOL3>(in, n, out, st); break;
    case FAM_CHOL6: launch<FAM_CHOL6>(in, n, out, st); break;
    case FAM_CHOL7: launch<FAM_CHOL7>(in, n, out, st); break;
    case FAM_CHOL4: launch<FAM_CHOL4>(in, n, out, st); break;
    case FAM_ROW: launch<FAM_ROW>(in, n, out, st); break;
    default: launch<FAM_ARM>(in, n, out, st); break;
  }
  return jh_launch_done(nullptr, st);
}
