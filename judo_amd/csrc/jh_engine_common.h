// jh_engine_common.h -- device helpers shared by the articulated-body kernels (gfx950): the model image's layout and view (jh_image.h), small vector algebra, MuJoCo's impedance curve and contact-frame convention, the
// elliptic-cone cost/force/Hessian of one contact, and the leap_cube running cost.
#pragma once
#include "jh_image.h"
#include "jh_internal.h"

namespace jh_eng {

template <int NM_, int NV_, int NQ_, int NU_, int NBLK_, int BD_, int NCON_, int NS_>
struct Cfg {
  static constexpr int NM = NM_, NV = NV_, NQ = NQ_, NU = NU_, NBLK = NBLK_, BD = BD_, NCON = NCON_, NS = NS_, NX = NQ_ + NV_;
  static constexpr int TRI = BD_ * (BD_ + 1) / 2;
};
using LeapCfg = Cfg<17, 22, 23, 16, 4, 4, 32, 31>;
using Fr3Cfg = Cfg<10, 15, 16, 8, 1, 9, 64, 14>;

// ------------------------------------------------------------------------------------------------ small vector helpers
__device__ __forceinline__ float dot3(const float* a, const float* b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }
__device__ __forceinline__ void cross3(float* r, const float* a, const float* b) {
  float x = a[1] * b[2] - a[2] * b[1], y = a[2] * b[0] - a[0] * b[2], z = a[0] * b[1] - a[1] * b[0];
  r[0] = x; r[1] = y; r[2] = z;
}
__device__ __forceinline__ void mulMV(float* r, const float* R, const float* v) {  // r = R v (row-major 3x3)
  float x = R[0] * v[0] + R[1] * v[1] + R[2] * v[2], y = R[3] * v[0] + R[4] * v[1] + R[5] * v[2], z = R[6] * v[0] + R[7] * v[1] + R[8] * v[2];
  r[0] = x; r[1] = y; r[2] = z;
}
__device__ __forceinline__ void mulMTV(float* r, const float* R, const float* v) {  // r = R' v
  float x = R[0] * v[0] + R[3] * v[1] + R[6] * v[2], y = R[1] * v[0] + R[4] * v[1] + R[7] * v[2], z = R[2] * v[0] + R[5] * v[1] + R[8] * v[2];
  r[0] = x; r[1] = y; r[2] = z;
}
__device__ __forceinline__ void mulMM(float* C, const float* A, const float* B) {
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 3; j++) C[3 * i + j] = A[3 * i] * B[j] + A[3 * i + 1] * B[3 + j] + A[3 * i + 2] * B[6 + j];
}
__device__ __forceinline__ void quat2mat(float* R, const float* q) {
  float w = q[0], x = q[1], y = q[2], z = q[3];
  R[0] = 1 - 2 * (y * y + z * z); R[1] = 2 * (x * y - w * z); R[2] = 2 * (x * z + w * y);
  R[3] = 2 * (x * y + w * z); R[4] = 1 - 2 * (x * x + z * z); R[5] = 2 * (y * z - w * x);
  R[6] = 2 * (x * z - w * y); R[7] = 2 * (y * z + w * x); R[8] = 1 - 2 * (x * x + y * y);
}
__device__ __forceinline__ void col3(float* a, const float* R, int k) { a[0] = R[k]; a[1] = R[3 + k]; a[2] = R[6 + k]; }
__device__ __forceinline__ int tri(int i, int j) { return i * (i + 1) / 2 + j; }  // packed lower triangle, j <= i

__device__ __forceinline__ float impedance(const float* si, float dist) {
  float s0 = si[0], s1 = si[1], s2 = si[2], s3 = si[3], s4 = si[4];
  if (s0 == s1 || s2 <= 1e-15f) return 0.5f * (s0 + s1);
  float x = fabsf(dist / s2);
  if (x >= 1.f) return s1;
  if (x <= 0.f) return s0;
  float y;
  if (s4 == 1.f) y = x;
  else if (s4 == 2.f) y = (x <= s3) ? x * x / s3 : 1.f - (1.f - x) * (1.f - x) / (1.f - s3);
  else if (x <= s3) y = powf(x, s4) / powf(s3, s4 - 1.f);
  else y = 1.f - powf(1.f - x, s4) / powf(1.f - s3, s4 - 1.f);
  return s0 + y * (s1 - s0);
}

// Capsule (centre pc, unit axis, half length L) against a box: parameter t in (-L, L) of the point of the capsule's axis that is closest to the box, or a value
// >= L when the minimum sits at an end of the segment (the end spheres, which the callers test anyway, then have it).  The squared distance
// d(t)^2 = sum_k max(|c_k + t a_k| - h_k, 0)^2 (box frame) is convex in t and its derivative monotone: 24 bisection steps resolve t to L * 1e-7.
__device__ __forceinline__ float capsule_box_closest(const float* pb, const float* Rb, const float* hb, const float* pc, const float* axis, float L) {
  const float d0[3] = {pc[0] - pb[0], pc[1] - pb[1], pc[2] - pb[2]};
  float c[3], a[3]; mulMTV(c, Rb, d0); mulMTV(a, Rb, axis);
  auto slope = [&](float t) __attribute__((always_inline)) {
    float g = 0.f;
#pragma unroll
    for (int k = 0; k < 3; k++) {  // sk minus its clamp to [-hb, hb]: sk - hb above, sk + hb below, exactly zero inside (one v_med3_f32: the ternary form became two exec-masked regions per axis, 24 times per pair)
      const float sk = fmaf(t, a[k], c[k]); g = fmaf(sk - __builtin_amdgcn_fmed3f(sk, -hb[k], hb[k]), a[k], g); }
    return g;
  };
  float lo = -L, hi = L;
  if (slope(lo) >= 0.f || slope(hi) <= 0.f) return 2.f * L + 1.f;
  for (int it = 0; it < 24; it++) { const float t = 0.5f * (lo + hi); if (slope(t) < 0.f) lo = t; else hi = t; }
  const float t = 0.5f * (lo + hi);
  return fabsf(t) >= L * (1.f - 1e-6f) ? 2.f * L + 1.f : t;
}

// contact frame from the normal, tangents as MuJoCo's mju_makeFrame picks them
__device__ __forceinline__ void make_frame(float* fr) {
  float* x = fr; float* y = fr + 3; float* z = fr + 6;
  float nn = rsqrtf(dot3(x, x)); x[0] *= nn; x[1] *= nn; x[2] *= nn;
  if (x[1] < -0.5f || x[1] > 0.5f) { y[0] = 0; y[1] = 0; y[2] = 1; } else { y[0] = 0; y[1] = 1; y[2] = 0; }
  float dp = dot3(x, y); y[0] -= x[0] * dp; y[1] -= x[1] * dp; y[2] -= x[2] * dp;
  nn = rsqrtf(dot3(y, y)); y[0] *= nn; y[1] *= nn; y[2] *= nn;
  cross3(z, x, y);
}

// world-frame inertia application: r = (Rk diag(I) Rk') v
__device__ __forceinline__ void inertia_mul(float* r, const float* Rk, const float* di, const float* v) {
  float t[3]; mulMTV(t, Rk, v); t[0] *= di[0]; t[1] *= di[1]; t[2] *= di[2]; mulMV(r, Rk, t);
}

// The smallest squared tangential part that counts as one: the smallest normal fp32 number.  v_rsq_f32 flushes a denormal input to zero and returns infinity, which
// T = T2 * iT turned into an infinite T and a NaN force; a T2 below this (a tangential part under 1.1e-19) is the T == 0 case, as a T2 that underflowed to 0 always was.
constexpr float CONE_T2_MIN = 1.17549435e-38f;

// elliptic-cone contact: force = -ds/djar, cost s, Hessian block W (sym 3x3: 00,10,11,20,21,22)
__device__ __forceinline__ float cone_eval(const float* jar, const float* D, float Dm, float mu, float fri, float* f, float* W) {
  float U0 = jar[0] * mu, U1 = jar[1] * fri, U2 = jar[2] * fri;
  float N = U0, T2 = U1 * U1 + U2 * U2;
  float iT = T2 >= CONE_T2_MIN ? __frsqrt_rn(T2) : 0.f, T = T2 * iT;
  // (T >= 0 and mu > 0: the degenerate cases T == 0 of MuJoCo's zone tests -- top if N >= 0, bottom if N < 0 -- are the same two comparisons; spelled out as `||` of a second
  // clause they cost two exec-mask round trips each)
  if (N >= mu * T) { f[0] = f[1] = f[2] = 0.f; for (int k = 0; k < 6; k++) W[k] = 0.f; return 0.f; }
  if (mu * N + T <= 0.f) {
    f[0] = -D[0] * jar[0]; f[1] = -D[1] * jar[1]; f[2] = -D[2] * jar[2];
    W[0] = D[0]; W[1] = 0.f; W[2] = D[1]; W[3] = 0.f; W[4] = 0.f; W[5] = D[2];
    return 0.5f * (D[0] * jar[0] * jar[0] + D[1] * jar[1] * jar[1] + D[2] * jar[2] * jar[2]);
  }
  // middle zone: distance to the cone; a = unit tangential direction (a branch-free variant of this function measured slower)
  const float NT = N - mu * T, a1 = U1 * iT, a2 = U2 * iT;
  f[0] = -Dm * NT * mu; f[1] = -f[0] * a1 * fri; f[2] = -f[0] * a2 * fri;
  const float k1 = Dm * mu * mu, k2 = Dm * NT * mu * iT;
  const float h01 = -Dm * mu * a1, h02 = -Dm * mu * a2;
  const float h11 = k1 * a1 * a1 - k2 * (1.f - a1 * a1), h12 = (k1 + k2) * a1 * a2, h22 = k1 * a2 * a2 - k2 * (1.f - a2 * a2);
  W[0] = mu * Dm * mu; W[1] = fri * h01 * mu; W[2] = fri * h11 * fri; W[3] = fri * h02 * mu; W[4] = fri * h12 * fri; W[5] = fri * h22 * fri;
  return 0.5f * Dm * NT * NT;
}

// cone_eval in two steps, for callers that skip a separated contact (the top zone) before anything else: cone_top returns the zone test and keeps the quantities the
// other two zones need; cone_below is cone_eval's bottom / middle part, expression for expression.  The same values up to rounding, NOT the same bits: the compiler
// contracts each inlined copy into fma on its own (the test kernel's two copies differ in W's last bit on two cases of three, tests/test_gpu_solver_blocks.py)
struct ConeZ { float U1, U2, N, iT, T; };
__device__ __forceinline__ bool cone_top(const float* jar, float mu, float fri, ConeZ& z) {
  float U0 = jar[0] * mu, U1 = jar[1] * fri, U2 = jar[2] * fri;
  float N = U0, T2 = U1 * U1 + U2 * U2;
  float iT = T2 >= CONE_T2_MIN ? __frsqrt_rn(T2) : 0.f, T = T2 * iT;
  z.U1 = U1; z.U2 = U2; z.N = N; z.iT = iT; z.T = T;
  return N >= mu * T;
}
__device__ __forceinline__ void cone_below(const float* jar, const float* D, float Dm, float mu, float fri, const ConeZ& z, float* f, float* W) {
  const float N = z.N, T = z.T, iT = z.iT, U1 = z.U1, U2 = z.U2;
  if (mu * N + T <= 0.f) {
    f[0] = -D[0] * jar[0]; f[1] = -D[1] * jar[1]; f[2] = -D[2] * jar[2];
    W[0] = D[0]; W[1] = 0.f; W[2] = D[1]; W[3] = 0.f; W[4] = 0.f; W[5] = D[2];
    return;
  }
  const float NT = N - mu * T, a1 = U1 * iT, a2 = U2 * iT;
  f[0] = -Dm * NT * mu; f[1] = -f[0] * a1 * fri; f[2] = -f[0] * a2 * fri;
  const float k1 = Dm * mu * mu, k2 = Dm * NT * mu * iT;
  const float h01 = -Dm * mu * a1, h02 = -Dm * mu * a2;
  const float h11 = k1 * a1 * a1 - k2 * (1.f - a1 * a1), h12 = (k1 + k2) * a1 * a2, h22 = k1 * a2 * a2 - k2 * (1.f - a2 * a2);
  W[0] = mu * Dm * mu; W[1] = fri * h01 * mu; W[2] = fri * h11 * fri; W[3] = fri * h02 * mu; W[4] = fri * h12 * fri; W[5] = fri * h22 * fri;
}

// directional derivatives of one elliptic-cone contact's cost along jp at jar (the exact line search needs only these two scalars):
// middle zone s = 1/2 Dm e^2 with e = N - mu T  =>  s' = Dm e e',  s'' = Dm (e'^2 + e e''),  T' = (U.V)/T,  T'' = (|V|^2 - T'^2)/T.
// Branch-free: the three zones are evaluated side by side and selected (lanes of a wave sit in different zones anyway);
// Dm = D0 / (mu^2 (1 + mu^2)) is a per-contact constant supplied by the caller.
__device__ __forceinline__ void cone_dir(const float* jar, const float* jp, const float* D, float Dm, float mu, float fri, float* d1, float* d2) {
  const float U1 = jar[1] * fri, U2 = jar[2] * fri, N = jar[0] * mu, T2 = U1 * U1 + U2 * U2;
  const float iT = T2 >= CONE_T2_MIN ? __frsqrt_rn(T2) : 0.f, T = T2 * iT;
  const bool top = N >= mu * T;             // (T == 0: N >= 0, MuJoCo's degenerate top case)
  const bool bottom = mu * N + T <= 0.f;    // (T == 0: N <= 0; N == 0 is `top`, which the selects below test first)
  const float b1 = D[0] * jar[0] * jp[0] + D[1] * jar[1] * jp[1] + D[2] * jar[2] * jp[2];
  const float b2 = D[0] * jp[0] * jp[0] + D[1] * jp[1] * jp[1] + D[2] * jp[2] * jp[2];
  const float V0 = jp[0] * mu, V1 = jp[1] * fri, V2 = jp[2] * fri, e = N - mu * T;
  const float Tp = (U1 * V1 + U2 * V2) * iT, Tpp = (V1 * V1 + V2 * V2 - Tp * Tp) * iT, ep = V0 - mu * Tp;
  float m1 = Dm * e * ep, m2 = Dm * (ep * ep - e * mu * Tpp), c1 = b1, c2 = b2;
  asm volatile("" : "+v"(m1), "+v"(m2), "+v"(c1), "+v"(c2));  // all three zones are evaluated: the selects below stay selects (left to itself the compiler branches around them)
  *d1 += top ? 0.f : (bottom ? c1 : m1);
  *d2 += top ? 0.f : (bottom ? c2 : m2);
}

// pyramidal-cone contact (condim 3): four one-sided rows  jar_n +- mu*jar_t1, jar_n +- mu*jar_t2, all with the same D.
// Expressed in the contact-frame 3-vector jar = J a - aref it returns the frame force f = -ds/djar and the 3x3 weight W.
__device__ __forceinline__ float pyramid_eval(const float* jar, float D, float mu, float* f, float* W) {
  float cs = 0.f, fn = 0.f, f1 = 0.f, f2 = 0.f, w00 = 0.f, w01 = 0.f, w02 = 0.f, w11 = 0.f, w22 = 0.f;
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const float sg = (k & 1) ? -mu : mu;
    const float x = jar[0] + sg * (k < 2 ? jar[1] : jar[2]);
    if (x < 0.f) {
      cs += 0.5f * D * x * x; const float fk = -D * x;
      fn += fk; w00 += D;
      if (k < 2) { f1 += sg * fk; w01 += sg * D; w11 += sg * sg * D; } else { f2 += sg * fk; w02 += sg * D; w22 += sg * sg * D; }
    }
  }
  f[0] = fn; f[1] = f1; f[2] = f2;
  W[0] = w00; W[1] = w01; W[2] = w11; W[3] = w02; W[4] = 0.f; W[5] = w22;
  return cs;
}
__device__ __forceinline__ float contact_eval(int cone, const float* jar, const float* D, float mu, float fri, float* f, float* W) {
  return cone == 1 ? cone_eval(jar, D, D[0] * __frcp_rn(mu * mu * (1.f + mu * mu)), mu, fri, f, W) : pyramid_eval(jar, D[0], fri, f, W);
}

// ------------------------------------------------------------------------------------------------ task costs
// leap_cube (judo/tasks/leap_cube.py:63-88): tp = (w_pos, w_rot, goal_pos[3], goal_quat[4]); MEAN over time
__device__ __forceinline__ float leap_step_cost(const float* tp, const float* qpos) {
  float d0 = qpos[0] - tp[2], d1 = qpos[1] - tp[3], d2 = qpos[2] - tp[4];
  const float* v = tp + 5;
  float u0 = qpos[3], u1 = -qpos[4], u2 = -qpos[5], u3 = -qpos[6];
  float ww = u0 * v[0] - u1 * v[1] - u2 * v[2] - u3 * v[3];
  float x = u0 * v[1] + u1 * v[0] + u2 * v[3] - u3 * v[2];
  float y = u0 * v[2] - u1 * v[3] + u2 * v[0] + u3 * v[1];
  float z = u0 * v[3] + u1 * v[2] - u2 * v[1] + u3 * v[0];
  float sn = sqrtf(x * x + y * y + z * z);
  float speed = 2.f * atan2f(sn, ww);
  if (speed > 3.14159265358979f) speed -= 6.28318530717959f;
  // |axis| = 1 in both branches of safe_normalize_axis, so |log map|^2 = speed^2
  return tp[0] * 0.5f * (d0 * d0 + d1 * d1 + d2 * d2) + tp[1] * 0.5f * speed * speed;
}


// fr3_pick (judo/tasks/fr3_pick.py:225-311): one step's contribution.  tp = (w_lift_close, w_lift_height, w_move_goal, w_move_close,
// w_place_table, w_place_goal, w_upright, w_coll, w_qvel, w_open, goal_x, goal_y, pick_height, arm_home[9]).  `y` = sensordata of the forward
// pass that produced the state (it lags the state by one step, as in the reference); `decay` = linspace(1,0,H)[h].
// Which of fr3_pick's five distance sensors (sensordata 0..4: left / right finger - object, left / right finger - table, object - table; fr3_pick.xml, checked by
// jh_model_is_fr3) fr3_step_cost below READS, and how: kept next to it so that an edit of the cost cannot leave a kernel shortcut behind.
//   y[0], y[1]  never read;  y[2], y[3]  only as `<= 0` (the sign);  y[4]  only in phase 2 (PLACE), by value.
constexpr int FR3_Y_FINGER_TABLE_L = 2, FR3_Y_FINGER_TABLE_R = 3, FR3_Y_OBJ_TABLE = 4, FR3_NDIST = 5, FR3_PHASE_PLACE = 2;
__host__ __device__ __forceinline__ bool fr3_cost_reads_distance(int adr, int phase) { return adr == FR3_Y_FINGER_TABLE_L || adr == FR3_Y_FINGER_TABLE_R || (adr == FR3_Y_OBJ_TABLE && phase == FR3_PHASE_PLACE); }
__host__ __device__ __forceinline__ bool fr3_cost_reads_sign_only(int adr) { return adr == FR3_Y_FINGER_TABLE_L || adr == FR3_Y_FINGER_TABLE_R; }
__device__ __forceinline__ float fr3_step_cost(const float* tp, int phase, const float* qpos, const float* qvel, int nv, const float* y, float decay) {
  const float* gs = y + 11; const float* ez = y + 5;
  float gd = (gs[0] - qpos[0]) * (gs[0] - qpos[0]) + (gs[1] - qpos[1]) * (gs[1] - qpos[1]) + (gs[2] - qpos[2]) * (gs[2] - qpos[2]);
  float he = (qpos[2] - tp[12]) * (qpos[2] - tp[12]);
  float og = sqrtf((qpos[0] - tp[10]) * (qpos[0] - tp[10]) + (qpos[1] - tp[11]) * (qpos[1] - tp[11]));
  float c;
  if (phase == 0) c = tp[0] * gd + tp[1] * he;
  else if (phase == 1) c = tp[2] * og + tp[3] * gd;
  else if (phase == FR3_PHASE_PLACE) c = tp[4] * y[FR3_Y_OBJ_TABLE] + tp[5] * og;
  else { float hd = 0.f; for (int k = 0; k < 9; k++) hd += (qpos[7 + k] - tp[13 + k]) * (qpos[7 + k] - tp[13 + k]); c = sqrtf(hd); }
  float up = sqrtf(ez[0] * ez[0] + ez[1] * ez[1] + (ez[2] + 1.f) * (ez[2] + 1.f));
  float touching = (y[FR3_Y_FINGER_TABLE_L] <= 0.f || y[FR3_Y_FINGER_TABLE_R] <= 0.f) ? 1.f : 0.f;
  float qn = 0.f; for (int k = 0; k < nv; k++) qn += qvel[k] * qvel[k];
  float op = (qpos[15] - 0.04f) * (qpos[15] - 0.04f);
  // reward = -(phase terms) + w_upright*(-up) + w_coll*(1-touching) + w_qvel*(-decay*|qvel|) + w_open*(-op); cost = -reward
  return c + tp[6] * up - tp[7] * (1.f - touching) + tp[8] * decay * sqrtf(qn) + tp[9] * op;
}

}  // namespace jh_eng
