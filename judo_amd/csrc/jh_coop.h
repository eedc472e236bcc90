// jh_coop.h -- building blocks of the cooperative (16 lanes per rollout) engine kernels on gfx950: row-local DPP reductions and
// the buffer-free box-box / box-sphere narrow phase that feeds a caller-supplied contact sink.
#pragma once
#include <type_traits>
#include <utility>

#include "jh_engine_common.h"

namespace jh_coop {
using namespace jh_eng;

// Cross-lane traffic stays inside one DPP row (the 16 lanes of a rollout): row-local DPP modifiers instead of
// ds_bpermute.  A sum butterfly only needs each step to pair a lane with one from the "other half" of the group that is
// already uniform: quad_perm xor 1, quad_perm xor 2, row_half_mirror (i <-> 7-i), row_mirror (i <-> 15-i).
template <int CTRL>
__device__ __forceinline__ float dppf(float v) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xF, 0xF, true));
}
template <int CTRL>
__device__ __forceinline__ int dppi(int v) { return __builtin_amdgcn_update_dpp(0, v, CTRL, 0xF, 0xF, true); }
constexpr int DPP_XOR1 = 0xB1, DPP_XOR2 = 0x4E, DPP_HALF_MIRROR = 0x141, DPP_MIRROR = 0x140;
// lane N of each DPP row to all 16 lanes of that row (row_newbcast:N, gfx90a and later): one VALU operand modifier, no LDS round trip
template <int N>
__device__ __forceinline__ float row_bcast(float v) { return dppf<0x150 + N>(v); }

// The sums must come out bit-identical in every lane of the group (the lanes of a rollout take the same branches on them, e.g. the
// line-search step).  With -ffp-contract the compiler may fuse the multiply that produced `v` into the first butterfly add,
// fma(x_i, y_i, round(x_j y_j)) in lane i against fma(x_j, y_j, round(x_i y_i)) in lane j: not the same number.  The empty asm makes
// `v` an opaque, already rounded register value, so every step is a plain commutative add.
__device__ __forceinline__ float csum(float v) {  // sum over the 4 lanes of a chain (= one quad)
  asm volatile("" : "+v"(v));
  v += dppf<DPP_XOR1>(v); v += dppf<DPP_XOR2>(v);
  return v;
}
__device__ __forceinline__ float gsum(float v) {  // sum over the 16 lanes of a rollout (= one DPP row)
  v = csum(v); v += dppf<DPP_HALF_MIRROR>(v); v += dppf<DPP_MIRROR>(v);
  return v;
}
// sum over the four chains (quads) of a rollout for the same position inside the quad: lanes l, l+4, l+8, l+12 of the row (row rotations by 4 and 8)
__device__ __forceinline__ float qsum4(float v) {
  asm volatile("" : "+v"(v));
  v += dppf<0x124>(v); v += dppf<0x128>(v);
  return v;
}
// the same sum with the rotation by 8 first: lanes c and c+2 then hold the same pair sum (a + b = b + a bit for bit), and the rotation by 4 adds the two pair sums in
// either order -- the result is bit-identical in all four lanes (qsum4's order gives four different associations), which a value every lane branches or solves on needs
__device__ __forceinline__ float qsum4_same(float v) {
  asm volatile("" : "+v"(v));
  v += dppf<0x128>(v); v += dppf<0x124>(v);
  return v;
}
// sum over the rollout's 16 lanes of SIXTEEN values at once, lane l receiving the sum of v[l] (a reduce-scatter): at each of four steps a lane keeps the half of its
// values whose index shares its next lane bit and adds the partner's copy of that half -- mirror, half mirror, xor 2, xor 1 pair lanes that differ in that bit and hold
// the same index set.  45 instructions (15 DPP adds, 30 selects) instead of 64 DPP adds + 16 selects for sixteen all-lane sums of which every lane keeps one.
__device__ __forceinline__ float row_scatter16(const float* v, int l) {
  const bool b3 = (l & 8) != 0, b2 = (l & 4) != 0, b1 = (l & 2) != 0, b0 = (l & 1) != 0;
  float k8[8], k4[4], k2[2];
#pragma unroll
  for (int j = 0; j < 8; j++) { const float keep = b3 ? v[8 + j] : v[j], send = b3 ? v[j] : v[8 + j]; k8[j] = keep + dppf<DPP_MIRROR>(send); }
#pragma unroll
  for (int j = 0; j < 4; j++) { const float keep = b2 ? k8[4 + j] : k8[j], send = b2 ? k8[j] : k8[4 + j]; k4[j] = keep + dppf<DPP_HALF_MIRROR>(send); }
#pragma unroll
  for (int j = 0; j < 2; j++) { const float keep = b1 ? k4[2 + j] : k4[j], send = b1 ? k4[j] : k4[2 + j]; k2[j] = keep + dppf<DPP_XOR2>(send); }
  return (b0 ? k2[1] : k2[0]) + dppf<DPP_XOR1>(b0 ? k2[0] : k2[1]);
}
__device__ __forceinline__ int gor(int v) {
  v |= dppi<DPP_XOR1>(v); v |= dppi<DPP_XOR2>(v); v |= dppi<DPP_HALF_MIRROR>(v); v |= dppi<DPP_MIRROR>(v);
  return v;
}
__device__ __forceinline__ int gmini(int v) {  // min over the 16 lanes of a rollout (signed)
  v = min(v, dppi<DPP_XOR1>(v)); v = min(v, dppi<DPP_XOR2>(v)); v = min(v, dppi<DPP_HALF_MIRROR>(v)); v = min(v, dppi<DPP_MIRROR>(v));
  return v;
}
// value held by lane j of the caller's quad (j is a compile-time constant after unrolling)
__device__ __forceinline__ float quad_get(float v, int j) {
  switch (j) { case 0: return dppf<0x00>(v); case 1: return dppf<0x55>(v); case 2: return dppf<0xAA>(v); default: return dppf<0xFF>(v); }
}

// min over the 16 lanes of a rollout.  fminf IGNORES a NaN lane: the result is the minimum of the lanes that hold numbers, and a NaN only when all 16 lanes are NaN --
// a caller that must see a NaN has to test for it itself
__device__ __forceinline__ float gmin(float v) {
  v = fminf(v, dppf<DPP_XOR1>(v)); v = fminf(v, dppf<DPP_XOR2>(v)); v = fminf(v, dppf<DPP_HALF_MIRROR>(v)); v = fminf(v, dppf<DPP_MIRROR>(v));
  return v;
}

// ---- small dense blocks in registers (packed lower-triangular, compile-time indices only).  A wave that runs alone on its SIMD pays every LDS round
// trip and barrier in full, so blocks of up to ~9 x 9 are cheaper to factorise redundantly in every lane than to pass pivot rows through LDS.
__host__ __device__ constexpr int tri4(int p, int m) { return p * (p + 1) / 2 + m; }

// In-place Cholesky of an N x N block held as packed lower-triangular registers; the diagonal slots end up holding 1 / L_pp.
template <int N>
__device__ __forceinline__ void chol_packed(float* a) {
#pragma unroll
  for (int p = 0; p < N; p++) {
#pragma unroll
    for (int m = 0; m < p; m++) {
      float s = a[tri4(p, m)];
#pragma unroll
      for (int q = 0; q < m; q++) s -= a[tri4(p, q)] * a[tri4(m, q)];
      a[tri4(p, m)] = s * a[tri4(m, m)];
    }
    float d = a[tri4(p, p)];
#pragma unroll
    for (int q = 0; q < p; q++) d -= a[tri4(p, q)] * a[tri4(p, q)];
    a[tri4(p, p)] = __frsqrt_rn(fmaxf(d, 1e-30f));
  }
}
// v <- v L^-T restricted to one block: forward substitution of a row segment through the block's factor
template <int N>
__device__ __forceinline__ void fwd_packed(float* v, const float* L) {
#pragma unroll
  for (int m = 0; m < N; m++) {
    float s = v[m];
#pragma unroll
    for (int q = 0; q < m; q++) s -= v[q] * L[tri4(m, q)];
    v[m] = s * L[tri4(m, m)];
  }
}

// x <- L^-T x for a factor from chol_packed (back substitution)
template <int N>
__device__ __forceinline__ void bwd_packed(float* v, const float* L) {
#pragma unroll
  for (int m = N - 1; m >= 0; m--) {
    float s = v[m];
#pragma unroll
    for (int q = m + 1; q < N; q++) s -= L[tri4(q, m)] * v[q];
    v[m] = s * L[tri4(m, m)];
  }
}

// 4x4 Cholesky (packed lower) + triangular solves on registers; the diagonal is kept as its reciprocal (one v_rsq per pivot, no divisions in the solves)
__device__ __forceinline__ void chol4(float* L, float* inv) {
#pragma unroll
  for (int i = 0; i < 4; i++)
#pragma unroll
    for (int j = 0; j <= i; j++) {
      float s = L[tri(i, j)];
#pragma unroll
      for (int k = 0; k < j; k++) s -= L[tri(i, k)] * L[tri(j, k)];
      if (i == j) { float r = __frsqrt_rn(fmaxf(s, 1e-30f)); inv[i] = r; L[tri(i, i)] = s * r; }
      else L[tri(i, j)] = s * inv[j];
    }
}
__device__ __forceinline__ void fwd4(const float* L, const float* inv, float* x) {
#pragma unroll
  for (int i = 0; i < 4; i++) { float s = x[i];
#pragma unroll
    for (int k = 0; k < i; k++) s -= L[tri(i, k)] * x[k];
    x[i] = s * inv[i]; }
}
__device__ __forceinline__ void bwd4(const float* L, const float* inv, float* x) {
#pragma unroll
  for (int i = 3; i >= 0; i--) { float s = x[i];
#pragma unroll
    for (int k = i + 1; k < 4; k++) s -= L[tri(k, i)] * x[k];
    x[i] = s * inv[i]; }
}

// dense Cholesky + solve of an n x n system held in registers (packed lower L, reciprocal diagonal), redundantly per lane
template <int N_>
__device__ __forceinline__ void chol_solve(float* L, float* x) {
  float inv[N_];
#pragma unroll
  for (int i = 0; i < N_; i++)
#pragma unroll
    for (int j = 0; j <= i; j++) {
      float s = L[tri(i, j)];
#pragma unroll
      for (int k = 0; k < j; k++) s -= L[tri(i, k)] * L[tri(j, k)];
      if (i == j) { float rr = __frsqrt_rn(fmaxf(s, 1e-30f)); inv[i] = rr; L[tri(i, i)] = s * rr; }
      else L[tri(i, j)] = s * inv[j];
    }
#pragma unroll
  for (int i = 0; i < N_; i++) { float s = x[i];
#pragma unroll
    for (int k = 0; k < i; k++) s -= L[tri(i, k)] * x[k];
    x[i] = s * inv[i]; }
#pragma unroll
  for (int i = N_ - 1; i >= 0; i--) { float s = x[i];
#pragma unroll
    for (int k = i + 1; k < N_; k++) s -= L[tri(k, i)] * x[k];
    x[i] = s * inv[i]; }
}

template <int N, class F, int... I>
__device__ __forceinline__ void static_for_impl(F&& f, std::integer_sequence<int, I...>) { (f(std::integral_constant<int, I>{}), ...); }
template <int N, class F>
__device__ __forceinline__ void static_for(F&& f) { static_for_impl<N>(f, std::make_integer_sequence<int, N>{}); }  // f(integral_constant<int, 0>) ... f(<N - 1>): compile-time indices for DPP controls

// The arm's 9 x 9 system with its rows spread over the arm's lanes (lane 6 + a holds row a, entries b <= a; lane 15 the right-hand side as a tenth row): right-looking
// Cholesky and both triangular solves with DPP row broadcasts, every entry receiving its subtractions in the order of chol_solve<9>; every lane gets x, bit for bit the
// same.  Not chol_solve<9>'s bits, though: the subtractions here are explicit fma, chol_solve's `s -= a * b` are contracted as the compiler sees fit (where it packs the
// multiplies in pairs the subtractions stay apart), so the two agree to rounding only (tests/test_gpu_solver_blocks.py holds both to the same residual).
// Replaces the factorisation every lane did redundantly on its own copy of the 45 entries.
template <int NA = 9>
__device__ __forceinline__ void arm_chol_solve(float* R, float* x, int l) {
  static_for<NA>([&](auto kc) {
    constexpr int k = decltype(kc)::value;
    const float rinv = __frsqrt_rn(fmaxf(row_bcast<6 + k>(R[k]), 1e-30f));
    const float lk = R[k] * rinv;
    R[k] = l == 6 + k ? rinv : lk;
    static_for<NA - 1 - k>([&](auto jc) {
      constexpr int j = k + 1 + decltype(jc)::value;
      R[j] = __builtin_fmaf(-lk, row_bcast<6 + j>(lk), R[j]);
    });
  });
  static_for<NA>([&](auto kc) {
    constexpr int k = NA - 1 - decltype(kc)::value;
    float s = row_bcast<15>(R[k]);
    static_for<NA - 1 - k>([&](auto jc) {
      constexpr int j = k + 1 + decltype(jc)::value;
      s = __builtin_fmaf(-row_bcast<6 + j>(R[k]), x[j], s);
    });
    x[k] = s * row_bcast<6 + k>(R[k]);
  });
}

// box-box contacts, normal from box 1 to box 2 (same algorithm as jh_engine.hip / the oracle); every contact goes to sk.push(pos, normal, dist)
// element / row i (0..2, a run-time value) of a register array, and the triple rotated to start at i: compare-and-select instead of
// an indexed read, so that the arrays stay in registers (an indexed read, or picking between two arrays through a pointer, puts them
// in scratch memory: one lane's box-box call then costs a round trip through memory per operand)
// (the empty asm pins the candidates in registers first: otherwise the compiler folds the select of three loads back into one load
// from a computed address, which is exactly the indexed scratch access this is meant to avoid)
__device__ __forceinline__ float pick(const float* a, int i) {
  float a0 = a[0], a1 = a[1], a2 = a[2];
#ifndef JH_PICK_NOASM
  asm volatile("" : "+v"(a0), "+v"(a1), "+v"(a2));
#endif
  return i == 0 ? a0 : (i == 1 ? a1 : a2);
}
__device__ __forceinline__ void pick_row(float* o, const float (*M)[3], int i) {
  for (int k = 0; k < 3; k++) {
    float m0 = M[0][k], m1 = M[1][k], m2 = M[2][k];
#ifndef JH_PICK_NOASM
    asm volatile("" : "+v"(m0), "+v"(m1), "+v"(m2));
#endif
    o[k] = i == 0 ? m0 : (i == 1 ? m1 : m2);
  }
}

template <class Sink>
__device__ __forceinline__ void collide_box_box(Sink& sk, const float* p1, const float* R1, const float* h1, const float* p2, const float* R2, const float* h2) {
  float A[3][3], B[3][3], dv[3], Cm[3][3], AC[3][3], dA[3], dB[3];
  for (int k = 0; k < 3; k++) { col3(A[k], R1, k); col3(B[k], R2, k); dv[k] = p2[k] - p1[k]; }
  for (int i = 0; i < 3; i++) { dA[i] = dot3(dv, A[i]); dB[i] = dot3(dv, B[i]); for (int j = 0; j < 3; j++) { Cm[i][j] = dot3(A[i], B[j]); AC[i][j] = fabsf(Cm[i][j]); } }
  // The fifteen separating-axis tests without an exit per axis: one flag, one exit.  (A candidate pair that reaches the narrow phase almost always touches, so the early exits
  // saved nothing -- and every one of them was an exec-mask round trip and a branch; lanes of a wave sit in different pairs anyway.)  Selects throughout: the same values.
  float best = -1e30f; int btype = -1, bi = 0, bj = 0; bool sep = false;
#pragma unroll
  for (int i = 0; i < 3; i++) {
    const float s = fabsf(dA[i]) - (h1[i] + h2[0] * AC[i][0] + h2[1] * AC[i][1] + h2[2] * AC[i][2]);
    sep = sep | (s > 0.f);
    const bool up = s > best; best = up ? s : best; btype = up ? 0 : btype; bi = up ? i : bi;
  }
#pragma unroll
  for (int j = 0; j < 3; j++) {
    const float s = fabsf(dB[j]) - (h2[j] + h1[0] * AC[0][j] + h1[1] * AC[1][j] + h1[2] * AC[2][j]);
    sep = sep | (s > 0.f);
    const bool up = s > best; best = up ? s : best; btype = up ? 1 : btype; bj = up ? j : bj;
  }
  float ebest = -1e30f, eL[3] = {0, 0, 0}; int ei = -1, ej = -1;
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 3; j++) {
      float L[3]; cross3(L, A[i], B[j]);
      const float l2 = dot3(L, L);
      const bool okl = !(l2 < 1e-12f);  // (parallel edges: no axis)
      const float il = rsqrtf(okl ? l2 : 1.f); L[0] *= il; L[1] *= il; L[2] *= il;
      float ra = 0.f, rb = 0.f;
      for (int k = 0; k < 3; k++) { ra += h1[k] * fabsf(dot3(A[k], L)); rb += h2[k] * fabsf(dot3(B[k], L)); }
      const float s = fabsf(dot3(dv, L)) - (ra + rb);
      sep = sep | (okl & (s > 0.f));
      const bool up = okl & (s > ebest);
      ebest = up ? s : ebest; ei = up ? i : ei; ej = up ? j : ej; eL[0] = up ? L[0] : eL[0]; eL[1] = up ? L[1] : eL[1]; eL[2] = up ? L[2] : eL[2];
    }
  if (sep) return;
  bool use_edge = ei >= 0 && (best < 0.f ? ebest > best / 1.05f + 1e-12f : ebest > best * 1.05f + 1e-12f);
  if (use_edge) {
    float n[3] = {eL[0], eL[1], eL[2]};
    if (dot3(n, dv) < 0.f) { n[0] = -n[0]; n[1] = -n[1]; n[2] = -n[2]; }
    float pa[3] = {p1[0], p1[1], p1[2]}, pb[3] = {p2[0], p2[1], p2[2]};
    for (int k = 0; k < 3; k++) {
      if (k != ei) { float s = (dot3(n, A[k]) > 0.f ? 1.f : -1.f) * h1[k]; pa[0] += A[k][0] * s; pa[1] += A[k][1] * s; pa[2] += A[k][2] * s; }
      if (k != ej) { float s = (dot3(n, B[k]) > 0.f ? -1.f : 1.f) * h2[k]; pb[0] += B[k][0] * s; pb[1] += B[k][1] * s; pb[2] += B[k][2] * s; }
    }
    float wv[3] = {pa[0] - pb[0], pa[1] - pb[1], pa[2] - pb[2]};
    float Ae[3], Be[3], Cme[3]; pick_row(Ae, A, ei); pick_row(Be, B, ej); pick_row(Cme, Cm, ei);
    const float h1e = pick(h1, ei), h2e = pick(h2, ej);
    float b = pick(Cme, ej), dd = dot3(Ae, wv), e = dot3(Be, wv), den = 1.f - b * b;
    float s = den > 1e-12f ? (b * e - dd) / den : 0.f, t = den > 1e-12f ? (e - b * dd) / den : 0.f;
    s = jh_clampf(s, -h1e, h1e); t = jh_clampf(t, -h2e, h2e);
    float pos[3];
    for (int k = 0; k < 3; k++) pos[k] = 0.5f * ((pa[k] + Ae[k] * s) + (pb[k] + Be[k] * t));
    sk.push(pos, n, ebest);
    return;
  }
  // reference box (owns the separating face) and incident box: values selected into registers
  const bool f0 = btype == 0;
  const int ri = f0 ? bi : bj;
  float pr[3], pi[3], hr[3], hi[3], Ar[3][3], Ai[3][3], n[3];
  for (int k = 0; k < 3; k++) {
    pr[k] = f0 ? p1[k] : p2[k]; pi[k] = f0 ? p2[k] : p1[k]; hr[k] = f0 ? h1[k] : h2[k]; hi[k] = f0 ? h2[k] : h1[k];
    for (int j = 0; j < 3; j++) { Ar[k][j] = f0 ? A[k][j] : B[k][j]; Ai[k][j] = f0 ? B[k][j] : A[k][j]; }
  }
  {
    float Arr[3]; pick_row(Arr, Ar, ri);
    const float dref = f0 ? pick(dA, bi) : pick(dB, bj);
    const float sg = f0 ? (dref >= 0.f ? 1.f : -1.f) : (dref >= 0.f ? -1.f : 1.f);
    for (int k = 0; k < 3; k++) n[k] = sg * Arr[k];
  }
  int mi = 0; float mb = -1.f;
  for (int k = 0; k < 3; k++) { float v = fabsf(dot3(n, Ai[k])); if (v > mb) { mb = v; mi = k; } }
  // Face manifold without polygon buffers: the vertices of (incident quad) n (reference rectangle) are exactly
  //   (a) incident vertices inside the rectangle, (b) incident-edge x rectangle-edge crossings, (c) rectangle corners inside the quad;
  // contact order is irrelevant, so they are emitted as found (same point set as Sutherland-Hodgman clipping).
  const int u = mi == 2 ? 0 : mi + 1, v = mi == 0 ? 2 : mi - 1, ra = ri == 2 ? 0 : ri + 1, rb = ri == 0 ? 2 : ri - 1;
  float Aim[3], Aiu[3], Aiv[3], Ara[3], Arb[3];
  pick_row(Aim, Ai, mi); pick_row(Aiu, Ai, u); pick_row(Aiv, Ai, v); pick_row(Ara, Ar, ra); pick_row(Arb, Ar, rb);
  const float him = pick(hi, mi), hiu = pick(hi, u), hiv = pick(hi, v);
  const float sgi = dot3(n, Aim) > 0.f ? -1.f : 1.f;
  const float ha = pick(hr, ra), hb = pick(hr, rb);
  float ci[3], e1[3], e2[3];
  for (int k = 0; k < 3; k++) { ci[k] = pi[k] + sgi * him * Aim[k] - pr[k]; e1[k] = hiu * Aiu[k]; e2[k] = hiv * Aiv[k]; }
  const float ca = dot3(ci, Ara), cbb = dot3(ci, Arb), cg = dot3(ci, n);
  const float e1a = dot3(e1, Ara), e1b = dot3(e1, Arb), e1g = dot3(e1, n), e2a = dot3(e2, Ara), e2b = dot3(e2, Arb), e2g = dot3(e2, n);
  const float href = pick(hr, ri);
  auto emit = [&](bool ok, float al, float be, float ga) __attribute__((always_inline)) {
    float depth = href - ga;
    if (!(ok & !(depth <= 0.f))) return;
    float pos[3], nn[3], gm = ga + 0.5f * depth;
    for (int k = 0; k < 3; k++) { pos[k] = pr[k] + al * Ara[k] + be * Arb[k] + gm * n[k]; nn[k] = f0 ? n[k] : -n[k]; }
    sk.push(pos, nn, -depth);
  };
  const float s1[4] = {1, -1, -1, 1}, s2[4] = {1, 1, -1, -1};
  float va[4], vb[4], vg[4];
#pragma unroll
  for (int q = 0; q < 4; q++) { va[q] = ca + s1[q] * e1a + s2[q] * e2a; vb[q] = cbb + s1[q] * e1b + s2[q] * e2b; vg[q] = cg + s1[q] * e1g + s2[q] * e2g; }
  // Degenerate alignments are the rule, not the exception, in the shipped models: the gripper's two pad stacks are mirror images (equal rectangles face to
  // face, vertices ON each other's edges), and in fp32 such a vertex lands exactly on the boundary in one coordinate and a few ulps outside in the other.
  // The three sets must therefore tile the boundary without a hole: (a) closed (<=), (b) open in the edge parameter but CLOSED in the other rectangle
  // coordinate, (c) open.  With (b) open in both, a vertex outside in `a` and exactly on `b = hb` belonged to no set: a closed gripper lost 8 of its 16
  // face-to-face pad contacts that way (found against the oracle's Sutherland-Hodgman clipping, which has no such hole).
#pragma unroll
  for (int q = 0; q < 4; q++) emit((fabsf(va[q]) <= ha) & (fabsf(vb[q]) <= hb), va[q], vb[q], vg[q]);   // (a)
#pragma unroll
  for (int q = 0; q < 4; q++) {                                                                        // (b)
    const int qn = (q + 1) & 3;
    const float da = va[qn] - va[q], db = vb[qn] - vb[q], dg = vg[qn] - vg[q];
#pragma unroll
    for (int sgn = -1; sgn <= 1; sgn += 2) {
      // (one predicate per crossing; with da == 0 the quotient is inf or nan and fails the comparisons by itself, the explicit test keeps the predicate what it was)
      { const float t = (sgn * ha - va[q]) / da, bb2 = vb[q] + t * db; emit((da != 0.f) & (t > 0.f) & (t < 1.f) & (fabsf(bb2) <= hb), sgn * ha, bb2, vg[q] + t * dg); }
      { const float t = (sgn * hb - vb[q]) / db, aa2 = va[q] + t * da; emit((db != 0.f) & (t > 0.f) & (t < 1.f) & (fabsf(aa2) <= ha), aa2, sgn * hb, vg[q] + t * dg); }
    }
  }
  const float det = e1a * e2b - e1b * e2a;                                                               // (c)
  if (fabsf(det) > 1e-12f) {
    const float idet = 1.f / det;
#pragma unroll
    for (int q = 0; q < 4; q++) {
      const float pa = s1[q] * ha - ca, pb2 = s2[q] * hb - cbb;
      const float t1 = (pa * e2b - pb2 * e2a) * idet, t2 = (e1a * pb2 - e1b * pa) * idet;
      emit((fabsf(t1) < 1.f) & (fabsf(t2) < 1.f), s1[q] * ha, s2[q] * hb, cg + t1 * e1g + t2 * e2g);
    }
  }
}

template <class Sink>
__device__ __forceinline__ void collide_box_sphere(Sink& sk, const float* pb, const float* Rb, const float* hb, const float* c, float r) {
  float dl[3] = {c[0] - pb[0], c[1] - pb[1], c[2] - pb[2]}, cl[3], q[3]; bool outside = false;
  mulMTV(cl, Rb, dl);
  for (int k = 0; k < 3; k++) { q[k] = cl[k]; if (q[k] > hb[k]) { q[k] = hb[k]; outside = true; } else if (q[k] < -hb[k]) { q[k] = -hb[k]; outside = true; } }
  float nl[3], dist;
  if (outside) {
    float df[3] = {cl[0] - q[0], cl[1] - q[1], cl[2] - q[2]}; float l = sqrtf(dot3(df, df));
    if (l - r >= 0.f) return;
    nl[0] = df[0] / l; nl[1] = df[1] / l; nl[2] = df[2] / l; dist = l - r;
  } else {
    int kb = 0; float mn = 1e30f;
    for (int k = 0; k < 3; k++) { float s = hb[k] - fabsf(cl[k]); if (s < mn) { mn = s; kb = k; } }
    for (int k = 0; k < 3; k++) { nl[k] = k == kb ? (cl[k] >= 0.f ? 1.f : -1.f) : 0.f; if (k == kb) q[k] = nl[k] * hb[k]; }  // no run-time array index: stays in registers
    dist = -mn - r;
  }
  float ql[3] = {q[0] + 0.5f * dist * nl[0], q[1] + 0.5f * dist * nl[1], q[2] + 0.5f * dist * nl[2]}, pos[3], n[3];
  mulMV(pos, Rb, ql); for (int k = 0; k < 3; k++) pos[k] += pb[k];
  mulMV(n, Rb, nl);
  sk.push(pos, n, dist);
}


// box against capsule (radius r, half length L along the local z of Rc): the two end spheres, and the point of the axis closest to the box when that lies strictly
// inside the segment (a capsule across an edge of the box); normal from the box to the capsule.  The fr3 links' stand-ins.
template <class Sink>
__device__ __forceinline__ void collide_box_capsule(Sink& sk, const float* pb, const float* Rb, const float* hb, const float* pc, const float* Rc, float r, float L) {
  float axis[3]; col3(axis, Rc, 2);
  const float tm = capsule_box_closest(pb, Rb, hb, pc, axis, L);
#pragma unroll 1
  for (int e = 0; e < 3; e++) {  // + end, - end, interior point (one copy of the box-sphere code)
    const float t = e == 0 ? L : (e == 1 ? -L : tm);
    if (e == 2 && tm > L) break;
    const float c[3] = {fmaf(t, axis[0], pc[0]), fmaf(t, axis[1], pc[1]), fmaf(t, axis[2], pc[2])};
    collide_box_sphere(sk, pb, Rb, hb, c, r);
  }
}

// capsule against capsule (MuJoCo's mjc_CapsuleCapsule as oracle/jo_engine.c::collide_capsule_capsule restates it; the shared routine: the fr3 kernel's self-collision build
// calls it, and jh_engine_v4.hip keeps a copy of its own inside its kernel for the Spot robot against itself, which compiles to the code it had): the closest points of the two axis segments, then sphere against
// sphere there; parallel axes: the ends of either capsule against the other's segment, at most two contacts.  Normal from the first capsule to the second.
template <class Sink>
__device__ __forceinline__ void collide_capsule_capsule(Sink& sk, const float* p1, const float* R1, float r1, float L1, const float* p2, const float* R2, float r2, float L2) {
  auto sphere_sphere = [&](const float* ca, const float* cb) __attribute__((always_inline)) {
    const float d[3] = {cb[0] - ca[0], cb[1] - ca[1], cb[2] - ca[2]}; const float ln = sqrtf(dot3(d, d)), dist = ln - r1 - r2;
    if (dist > 0.f) return false;
    const bool same = ln < 1e-12f;  // coincident centres: mju_normalize3 returns (1, 0, 0)
    const float n3[3] = {same ? 1.f : d[0] / ln, same ? 0.f : d[1] / ln, same ? 0.f : d[2] / ln}, mm = r1 + 0.5f * dist;
    const float ps[3] = {ca[0] + mm * n3[0], ca[1] + mm * n3[1], ca[2] + mm * n3[2]};
    sk.push(ps, n3, dist);
    return true;
  };
  float a1[3], a2[3]; col3(a1, R1, 2); col3(a2, R2, 2);
  for (int i = 0; i < 3; i++) { a1[i] *= L1; a2[i] *= L2; }
  const float dif[3] = {p1[0] - p2[0], p1[1] - p2[1], p1[2] - p2[2]};
  const float ma = dot3(a1, a1), mb = -dot3(a1, a2), mc = dot3(a2, a2), u = -dot3(a1, dif), v = dot3(a2, dif);
  const float det = ma * mc - mb * mb;
  if (fabsf(det) >= 1e-6f * ma * mc) {  // (MuJoCo: |det| >= mjMINVAL in fp64; in fp32 the determinant of two axes less than ~1e-3 rad apart is rounding noise)
    float x1 = (mc * u - mb * v) / det, x2 = (ma * v - mb * u) / det;
    if (x1 > 1.f) { x1 = 1.f; x2 = (v - mb) / mc; } else if (x1 < -1.f) { x1 = -1.f; x2 = (v + mb) / mc; }
    if (x2 > 1.f) { x2 = 1.f; x1 = jh_clampf((u - mb) / ma, -1.f, 1.f); }
    else if (x2 < -1.f) { x2 = -1.f; x1 = jh_clampf((u + mb) / ma, -1.f, 1.f); }
    const float v1[3] = {p1[0] + a1[0] * x1, p1[1] + a1[1] * x1, p1[2] + a1[2] * x1}, v2[3] = {p2[0] + a2[0] * x2, p2[1] + a2[1] * x2, p2[2] + a2[2] * x2};
    sphere_sphere(v1, v2);
  } else {
    int nfound = 0;
#pragma unroll 1
    for (int e = 0; e < 4; e++) {
      float x1, x2;
      if (e < 2) { x1 = e == 0 ? 1.f : -1.f; x2 = jh_clampf((v - x1 * mb) / mc, -1.f, 1.f); }
      else { x2 = e == 2 ? 1.f : -1.f; x1 = jh_clampf((u - x2 * mb) / ma, -1.f, 1.f); }
      const float v1[3] = {p1[0] + a1[0] * x1, p1[1] + a1[1] * x1, p1[2] + a1[2] * x1}, v2[3] = {p2[0] + a2[0] * x2, p2[1] + a2[1] * x2, p2[2] + a2[2] * x2};
      if (nfound < 2 && sphere_sphere(v1, v2)) nfound++;
    }
  }
}

// ---- a cylinder (radius r, half length L along the local z of Rc) against the robot's geoms: the spot_tire object (csrc/jh_engine_v4.hip, k_tree_v4<SELF, true, true>)

// sphere against cylinder (MuJoCo's primitive mjc_SphereCylinder, as the oracle restates it in collide_cylinder_sphere): the closest point of the solid cylinder to the
// centre (side, cap or rim), the normal from the cylinder to the sphere along that line, position midway through the overlap; a centre inside leaves through the nearer
// of side and cap
template <class Sink>
__device__ __forceinline__ void collide_cylinder_sphere(Sink& sk, const float* pc, const float* Rc, float r, float L, const float* ps, float rs) {
  float ax[3]; col3(ax, Rc, 2);
  const float v[3] = {ps[0] - pc[0], ps[1] - pc[1], ps[2] - pc[2]};
  const float x = dot3(v, ax);
  const float rad[3] = {v[0] - x * ax[0], v[1] - x * ax[1], v[2] - x * ax[2]};
  const float rl = sqrtf(dot3(rad, rad));
  float er[3];
  if (rl > 1e-7f) { er[0] = rad[0] / rl; er[1] = rad[1] / rl; er[2] = rad[2] / rl; }
  else {  // centre on the axis: any radial direction
    const float t[3] = {fabsf(ax[0]) > 0.9f ? 0.f : 1.f, fabsf(ax[0]) > 0.9f ? 1.f : 0.f, 0.f};
    cross3(er, ax, t); const float l = sqrtf(dot3(er, er)); er[0] /= l; er[1] /= l; er[2] /= l;
  }
  const float sx = x >= 0.f ? 1.f : -1.f;
  float n[3], cp[3], dist;
  if (fabsf(x) <= L && rl <= r) {  // centre inside
    const float dside = r - rl, dcap = L - fabsf(x);
    if (dside <= dcap) { for (int k = 0; k < 3; k++) { n[k] = er[k]; cp[k] = pc[k] + x * ax[k] + r * er[k]; } dist = -dside - rs; }
    else { for (int k = 0; k < 3; k++) { n[k] = sx * ax[k]; cp[k] = pc[k] + sx * L * ax[k] + rl * er[k]; } dist = -dcap - rs; }
  } else {
    const float cx = fabsf(x) > L ? sx * L : x, cr = rl > r ? r : rl;
    for (int k = 0; k < 3; k++) cp[k] = pc[k] + cx * ax[k] + cr * er[k];
    const float dv[3] = {ps[0] - cp[0], ps[1] - cp[1], ps[2] - cp[2]};
    const float l = sqrtf(dot3(dv, dv));
    if (l < 1e-7f) return;
    for (int k = 0; k < 3; k++) n[k] = dv[k] / l;
    dist = l - rs;
  }
  if (dist >= 0.f) return;
  const float pos[3] = {cp[0] + n[0] * 0.5f * dist, cp[1] + n[1] * 0.5f * dist, cp[2] + n[2] * 0.5f * dist};
  sk.push(pos, n, dist);
}

// A capsule (type 3) or a box (type 6) against the cylinder: MuJoCo sends these pairs through its general convex collider (mjc_Convex, GJK + EPA), which gives ONE contact
// of minimum translation -- depth, normal from geom 1 to geom 2, position midway between the two witness points.  The oracle restates it in double precision
// (collide_convex, oracle/jo_engine.c).  This is the same algorithm in fp32 with a BOUNDED polytope, chosen over exact special cases because box-cylinder has no closed form
// (its minimum translation can lie along a curved face of the Minkowski difference) and capsule-cylinder would need one per feature pair.  Worst case per lane: GJK at most
// CVX_GJK_IT = 48 support steps; EPA at most CVX_MAXV - 4 = 36 expansions of a polytope of at most CVX_MAXV = 40 vertices and 2 CVX_MAXV = 80 faces (a closed
// triangulation of V vertices has 2V - 4), each expansion O(faces).  The polytope lives in the lane's private memory (about 2.6 KB, scratch), not in LDS.  It stops when
// the closest face is a supporting plane within CVX_TOL = 1e-6 (m); a curved contact that needs more than 36 expansions keeps the closest face found so far, whose
// depth is then below the true one by less than the last expansion's growth.  Where the closest feature is not unique (parallel faces or edges) the witness points --
// and so the position -- may differ from the oracle's within that feature; the depth does not (measured within 1.3e-6 m of the oracle's).  The normal of a CURVED contact
// does: a supporting plane within the stop of a face of radius r may be tilted by sqrt(2 CVX_TOL / r), about 1e-2 at r = 20 mm (measured: up to 9.1e-3,
// profiles/narrow_phase_pairs.md); along the reported normal the shapes overlap by the reported depth to within the stop, which is what the solver needs.
constexpr int CVX_MAXV = 40, CVX_MAXF = 2 * CVX_MAXV, CVX_GJK_IT = 48;
constexpr float CVX_TOL = 1e-6f;
constexpr int CVX_STOP_NM = 1000;  // the stop of the leap cylinder build's GJK + EPA in nanometres (1 000 = CVX_TOL, the tree kernel's); profiles/caltech_cylinder.md has 1 000 against 100
struct CvxShape { int type; float s0, s1, s2; float p[3], R[9]; };
// The part of d across a cylinder's axis is made orthogonal to the axis a SECOND time.  For d within about 1e-5 rad of the axis that part is the rounding residue of d - (d . ax) ax, which is not orthogonal to
// the axis; scaled to the radius it puts the "support point" up to a quarter of a millimetre above the cap of a 14 mm cylinder, outside the shape, and the polytope
// built on it misses a minimum translation that runs along the axis (a cap contact).  A rim point in whatever direction the residue has is a valid support point.
// (This was a template switch that only the leap kernel's cylinder build turned on; the tree kernel ran without it until the routine was tested alone: against the 0.33 m tire it reported contacts up to 8 mm deeper than the shapes overlap,
// profiles/narrow_phase_pairs.md; EPA's face normals converge onto the cap's, so directions that close to the axis are the rule there.)
__device__ __forceinline__ void cvx_support(const CvxShape& s, const float* d, float* out) {
  out[0] = s.p[0]; out[1] = s.p[1]; out[2] = s.p[2];
  if (s.type == 6) {
    const float h[3] = {s.s0, s.s1, s.s2};
#pragma unroll
    for (int k = 0; k < 3; k++) {
      float ax[3]; col3(ax, s.R, k); const float e = dot3(d, ax) >= 0.f ? h[k] : -h[k];
      out[0] = fmaf(ax[0], e, out[0]); out[1] = fmaf(ax[1], e, out[1]); out[2] = fmaf(ax[2], e, out[2]);
    }
  } else {  // capsule or cylinder: the end of the axis segment that faces d, then the radius -- all of it (capsule) or its part across the axis (cylinder)
    float ax[3]; col3(ax, s.R, 2);
    const float da = dot3(d, ax), e = da >= 0.f ? s.s1 : -s.s1;
    out[0] = fmaf(ax[0], e, out[0]); out[1] = fmaf(ax[1], e, out[1]); out[2] = fmaf(ax[2], e, out[2]);
    float r[3] = {d[0], d[1], d[2]};
    if (s.type == 5) { r[0] -= da * ax[0]; r[1] -= da * ax[1]; r[2] -= da * ax[2]; }
    if (s.type == 5) { const float db = dot3(r, ax); r[0] -= db * ax[0]; r[1] -= db * ax[1]; r[2] -= db * ax[2]; }
    const float l = sqrtf(dot3(r, r));
    if (l > 1e-7f * (fabsf(da) + l)) { const float k = s.s0 / l; out[0] = fmaf(r[0], k, out[0]); out[1] = fmaf(r[1], k, out[1]); out[2] = fmaf(r[2], k, out[2]); }
  }
}
struct CvxVert { float w[3], a[3]; };  // w = a - b on the Minkowski difference A - B; a the support point of A (b follows)
__device__ __forceinline__ void cvx_vertex(const CvxShape& A, const CvxShape& B, const float* d, CvxVert& v) {
  const float nd[3] = {-d[0], -d[1], -d[2]};
  float b[3];
  cvx_support(A, d, v.a); cvx_support(B, nd, b);
  v.w[0] = v.a[0] - b[0]; v.w[1] = v.a[1] - b[1]; v.w[2] = v.a[2] - b[2];
}
struct CvxFace { float n[3], dist; int v; };  // v: vertex indices 0-7 / 8-15 / 16-23, bit 31 dead
__device__ __forceinline__ bool cvx_face(const CvxVert* V, int i, int j, int k, CvxFace& f) {
  const float e1[3] = {V[j].w[0] - V[i].w[0], V[j].w[1] - V[i].w[1], V[j].w[2] - V[i].w[2]}, e2[3] = {V[k].w[0] - V[i].w[0], V[k].w[1] - V[i].w[1], V[k].w[2] - V[i].w[2]};
  cross3(f.n, e1, e2);
  const float l = sqrtf(dot3(f.n, f.n));
  if (!(l > 1e-18f)) return false;
  f.n[0] /= l; f.n[1] /= l; f.n[2] /= l;
  f.dist = dot3(f.n, V[i].w);
  f.v = i | (j << 8) | (k << 16);
  if (f.dist < 0.f) { f.dist = -f.dist; f.n[0] = -f.n[0]; f.n[1] = -f.n[1]; f.n[2] = -f.n[2]; f.v = i | (k << 8) | (j << 16); }
  return true;
}
// GJK on A - B, overlap only (the oracle's ccd_gjk): true with four vertices around the origin in sx[0..3]
__device__ __forceinline__ bool cvx_gjk(const CvxShape& A, const CvxShape& B, CvxVert* sx) {
  float d[3] = {B.p[0] - A.p[0], B.p[1] - A.p[1], B.p[2] - A.p[2]};
  if (dot3(d, d) < 1e-20f) { d[0] = 1.f; d[1] = 0.f; d[2] = 0.f; }
  int n = 1;
  cvx_vertex(A, B, d, sx[0]);
  d[0] = -sx[0].w[0]; d[1] = -sx[0].w[1]; d[2] = -sx[0].w[2];
  for (int it = 0; it < CVX_GJK_IT; it++) {
    if (dot3(d, d) < 1e-24f) {  // the origin lies on the simplex: any direction that grows it
      float e[3] = {1.f, 0.f, 0.f};
      if (n >= 2) {
        const float ab[3] = {sx[1].w[0] - sx[0].w[0], sx[1].w[1] - sx[0].w[1], sx[1].w[2] - sx[0].w[2]};
        float t[3] = {0.f, 1.f, 0.f}; cross3(e, ab, t);
        if (dot3(e, e) < 1e-20f) { t[1] = 0.f; t[2] = 1.f; cross3(e, ab, t); }
      }
      d[0] = e[0]; d[1] = e[1]; d[2] = e[2];
    }
    CvxVert nv; cvx_vertex(A, B, d, nv);
    if (dot3(nv.w, d) < 0.f) return false;  // the new support point did not pass the origin: separated
    sx[3] = sx[2]; sx[2] = sx[1]; sx[1] = sx[0]; sx[0] = nv; n++;
    const float* a = sx[0].w; const float* b = sx[1].w;
    const float ao[3] = {-a[0], -a[1], -a[2]}, ab[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]};
    if (n == 2) {
      if (dot3(ab, ao) > 0.f) { float t[3]; cross3(t, ab, ao); cross3(d, t, ab); } else { n = 1; d[0] = ao[0]; d[1] = ao[1]; d[2] = ao[2]; }
    } else if (n == 3) {
      const float* c = sx[2].w;
      const float ac[3] = {c[0] - a[0], c[1] - a[1], c[2] - a[2]};
      float abc[3], t[3]; cross3(abc, ab, ac); cross3(t, abc, ac);
      if (dot3(t, ao) > 0.f) {
        if (dot3(ac, ao) > 0.f) { sx[1] = sx[2]; n = 2; float u[3]; cross3(u, ac, ao); cross3(d, u, ac); }
        else if (dot3(ab, ao) > 0.f) { n = 2; float u[3]; cross3(u, ab, ao); cross3(d, u, ab); }
        else { n = 1; d[0] = ao[0]; d[1] = ao[1]; d[2] = ao[2]; }
      } else {
        cross3(t, ab, abc);
        if (dot3(t, ao) > 0.f) {
          if (dot3(ab, ao) > 0.f) { n = 2; float u[3]; cross3(u, ab, ao); cross3(d, u, ab); } else { n = 1; d[0] = ao[0]; d[1] = ao[1]; d[2] = ao[2]; }
        } else if (dot3(abc, ao) > 0.f) { d[0] = abc[0]; d[1] = abc[1]; d[2] = abc[2]; }
        else { const CvxVert tmp = sx[1]; sx[1] = sx[2]; sx[2] = tmp; d[0] = -abc[0]; d[1] = -abc[1]; d[2] = -abc[2]; }
      }
    } else {  // tetrahedron: which face through the new vertex, if any, sees the origin
      const float* c = sx[2].w; const float* dd = sx[3].w;
      const float ac[3] = {c[0] - a[0], c[1] - a[1], c[2] - a[2]}, ad[3] = {dd[0] - a[0], dd[1] - a[1], dd[2] - a[2]};
      float abc[3], acd[3], adb[3]; cross3(abc, ab, ac); cross3(acd, ac, ad); cross3(adb, ad, ab);
      if (dot3(abc, ad) > 0.f) { abc[0] = -abc[0]; abc[1] = -abc[1]; abc[2] = -abc[2]; }
      if (dot3(acd, ab) > 0.f) { acd[0] = -acd[0]; acd[1] = -acd[1]; acd[2] = -acd[2]; }
      if (dot3(adb, ac) > 0.f) { adb[0] = -adb[0]; adb[1] = -adb[1]; adb[2] = -adb[2]; }
      if (dot3(abc, ao) > 0.f) { n = 3; d[0] = abc[0]; d[1] = abc[1]; d[2] = abc[2]; }
      else if (dot3(acd, ao) > 0.f) { sx[1] = sx[2]; sx[2] = sx[3]; n = 3; d[0] = acd[0]; d[1] = acd[1]; d[2] = acd[2]; }
      else if (dot3(adb, ao) > 0.f) { sx[2] = sx[1]; sx[1] = sx[3]; n = 3; d[0] = adb[0]; d[1] = adb[1]; d[2] = adb[2]; }
      else return true;
    }
  }
  return false;
}
// geom A (capsule / box) against geom B (the cylinder): at most one contact, normal from A to B.  (Either side may be a box, a capsule or a cylinder: the leap kernel's
// cylinder build calls it with the cylinder first, MuJoCo's order of a box-cylinder pair, and with two cylinders.)  STOP_NM: the stop in nanometres, CVX_TOL = 1 000 by default.
template <class Sink, int STOP_NM = 1000>
__device__ __noinline__ void collide_convex_cylinder(Sink& sk, const CvxShape& A, const CvxShape& B) {
  constexpr float STOP = STOP_NM == 1000 ? CVX_TOL : 1e-9f * (float)STOP_NM;
  CvxVert V[CVX_MAXV];
  CvxFace F[CVX_MAXF];
  int ed[CVX_MAXF];
  if (!cvx_gjk(A, B, V)) return;
  int nv = 4, nf = 0;
  {
    const int idx[4][3] = {{0, 1, 2}, {0, 2, 3}, {0, 3, 1}, {1, 3, 2}};
    for (int f = 0; f < 4; f++) {
      if (!cvx_face(V, idx[f][0], idx[f][1], idx[f][2], F[nf])) return;  // a flat simplex: touching without volume
      const int opp = 6 - idx[f][0] - idx[f][1] - idx[f][2];
      if (dot3(F[nf].n, V[opp].w) - F[nf].dist > 0.f) {  // the opposite vertex must lie behind the face
        F[nf].n[0] = -F[nf].n[0]; F[nf].n[1] = -F[nf].n[1]; F[nf].n[2] = -F[nf].n[2]; F[nf].dist = -F[nf].dist;
        F[nf].v = idx[f][0] | (idx[f][2] << 8) | (idx[f][1] << 16);
      }
      nf++;
    }
  }
  int best = -1;
  for (int it = 0; it < CVX_MAXV; it++) {
    best = -1;
    for (int f = 0; f < nf; f++) if (F[f].v >= 0 && (best < 0 || F[f].dist < F[best].dist)) best = f;
    if (best < 0) return;
    CvxVert nw; cvx_vertex(A, B, F[best].n, nw);
    if (dot3(nw.w, F[best].n) - F[best].dist < STOP || nv >= CVX_MAXV) break;
    int ne = 0;  // the faces the new point sees go; their unshared edges form the horizon
    for (int f = 0; f < nf; f++) {
      if (F[f].v < 0 || dot3(F[f].n, nw.w) - F[f].dist <= 0.f) continue;
      const int fv = F[f].v;
      F[f].v = fv | (1 << 31);
      for (int e = 0; e < 3; e++) {
        const int a = (fv >> (8 * e)) & 255, b = (fv >> (8 * ((e + 1) % 3))) & 255;
        int found = -1;
        for (int q = 0; q < ne; q++) if (ed[q] == (b | (a << 8))) { found = q; break; }
        if (found >= 0) ed[found] = ed[--ne];
        else if (ne < CVX_MAXF) ed[ne++] = a | (b << 8);
      }
    }
    if (ne == 0) break;  // numerically on the surface already
    V[nv] = nw;
    int k = 0;
    for (int f = 0; f < nf; f++) if (F[f].v >= 0) { if (k != f) F[k] = F[f]; k++; }
    nf = k;
    for (int e = 0; e < ne && nf < CVX_MAXF; e++) if (cvx_face(V, ed[e] & 255, ed[e] >> 8, nv, F[nf])) nf++;
    nv++;
    best = -1;
  }
  if (best < 0) return;
  const CvxFace f = F[best];
  const CvxVert& a = V[f.v & 255]; const CvxVert& b = V[(f.v >> 8) & 255]; const CvxVert& c = V[(f.v >> 16) & 255];
  const float pr[3] = {f.n[0] * f.dist, f.n[1] * f.dist, f.n[2] * f.dist};
  float v0[3], v1[3], v2[3];
  for (int k = 0; k < 3; k++) { v0[k] = b.w[k] - a.w[k]; v1[k] = c.w[k] - a.w[k]; v2[k] = pr[k] - a.w[k]; }
  const float d00 = dot3(v0, v0), d01 = dot3(v0, v1), d11 = dot3(v1, v1), d20 = dot3(v2, v0), d21 = dot3(v2, v1), den = d00 * d11 - d01 * d01;
  const float bv = den > 1e-30f ? (d11 * d20 - d01 * d21) / den : 0.f, bw = den > 1e-30f ? (d00 * d21 - d01 * d20) / den : 0.f, bu = 1.f - bv - bw;
  float pos[3];
  for (int k = 0; k < 3; k++) {  // midway between the witness points wa = sum a, wb = wa - sum w
    const float wa = bu * a.a[k] + bv * b.a[k] + bw * c.a[k], ww = bu * a.w[k] + bv * b.w[k] + bw * c.w[k];
    pos[k] = wa - 0.5f * ww;
  }
  sk.push(pos, f.n, -f.dist);
}

// signed box-box distance = largest separation over the 15 SAT axes (exact when a face or an edge pair is closest; see the oracle)
__device__ __forceinline__ float box_box_distance(const float* p1, const float* R1, const float* h1, const float* p2, const float* R2, const float* h2) {
  float A[3][3], B[3][3], dv[3], best = -1e30f;
  for (int k = 0; k < 3; k++) { col3(A[k], R1, k); col3(B[k], R2, k); dv[k] = p2[k] - p1[k]; }
  for (int i = 0; i < 3; i++) {
    float ra = h1[i], rb = 0.f; for (int k = 0; k < 3; k++) rb += h2[k] * fabsf(dot3(B[k], A[i]));
    float sA = fabsf(dot3(dv, A[i])) - ra - rb; if (sA > best) best = sA;
    ra = 0.f; rb = h2[i]; for (int k = 0; k < 3; k++) ra += h1[k] * fabsf(dot3(A[k], B[i]));
    float sB = fabsf(dot3(dv, B[i])) - ra - rb; if (sB > best) best = sB;
  }
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) {
      float L[3]; cross3(L, A[i], B[j]); float l2 = dot3(L, L);
      if (l2 < 1e-12f) continue;
      float il = rsqrtf(l2); L[0] *= il; L[1] *= il; L[2] *= il;
      float ra = 0.f, rb = 0.f; for (int k = 0; k < 3; k++) { ra += h1[k] * fabsf(dot3(A[k], L)); rb += h2[k] * fabsf(dot3(B[k], L)); }
      float sE = fabsf(dot3(dv, L)) - ra - rb; if (sE > best) best = sE;
    }
  return best;
}

// two boxes overlap or touch (box_box_distance(...) <= 0), decided at the first of the same 15 axes that separates them: what a cost term needs that only asks whether a
// distance sensor reads <= 0 (FR3Pick.reward's finger-table test, judo/tasks/fr3_pick.py:283-285) -- a pad above the table is done after a face axis or two
__device__ __forceinline__ bool box_box_touching(const float* p1, const float* R1, const float* h1, const float* p2, const float* R2, const float* h2) {
  float A[3][3], B[3][3], dv[3];
  for (int k = 0; k < 3; k++) { col3(A[k], R1, k); col3(B[k], R2, k); dv[k] = p2[k] - p1[k]; }
  bool apart = false;
#pragma unroll 1
  for (int i = 0; i < 3 && !apart; i++) {
    float ra = h1[i], rb = 0.f; for (int k = 0; k < 3; k++) rb += h2[k] * fabsf(dot3(B[k], A[i]));
    apart = fabsf(dot3(dv, A[i])) - ra - rb > 0.f;
    ra = 0.f; rb = h2[i]; for (int k = 0; k < 3; k++) ra += h1[k] * fabsf(dot3(A[k], B[i]));
    apart = apart || fabsf(dot3(dv, B[i])) - ra - rb > 0.f;
  }
#pragma unroll 1
  for (int ij = 0; ij < 9 && !apart; ij++) {
    const int i = ij / 3, j = ij - 3 * i;
    float Ai[3], Bj[3], L[3]; pick_row(Ai, A, i); pick_row(Bj, B, j); cross3(L, Ai, Bj); const float l2 = dot3(L, L);
    if (l2 < 1e-12f) continue;
    const float il = rsqrtf(l2); L[0] *= il; L[1] *= il; L[2] *= il;
    float ra = 0.f, rb = 0.f; for (int k = 0; k < 3; k++) { ra += h1[k] * fabsf(dot3(A[k], L)); rb += h2[k] * fabsf(dot3(B[k], L)); }
    apart = fabsf(dot3(dv, L)) - ra - rb > 0.f;
  }
  return !apart;
}

}  // namespace jh_coop
