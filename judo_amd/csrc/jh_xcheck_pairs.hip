// jh_xcheck_pairs.hip -- TEST BUILD ONLY (libjudo_amd_xcheck.so): the narrow-phase device routines of jh_coop.h, one pair of free-standing shapes per lane.
//
// The shipped kernels reach these routines only from inside a physics step, where a wrong contact is diluted by the solver and the branch a state reaches is not
// controlled.  This kernel calls one routine per launch on n independent pairs and writes every contact it pushes, so that tests/test_gpu_narrow_phase.py can hold each
// routine to exact geometry (tests/independent.py) and to the oracle's routine of the same name.  The instantiations are the shipped kernels' own (collide_convex_cylinder has one: both shipped callers stop at 1 000 nm); the file is compiled
// with the common flags (the engine files carry their own), so the comparison is to a tolerance, not to bits.
//
// Input: JH_PAIR_F floats per pair, two shapes of (type, size[3], pos[3], R[9] row-major); types are MuJoCo's (2 sphere, 3 capsule, 5 cylinder, 6 box).
// Output: JH_PAIR_ROWS rows of (pos[3], normal[3], dist) per pair and the RAW number of pushes (24 = the emit sites of collide_box_box: nothing can be dropped; the
// row index is clamped all the same).  Routine 6 writes box_box_distance into the pair's first float and box_box_touching into its count.
#include <hip/hip_runtime.h>

#include "jh_coop.h"

using namespace jh_eng;
using namespace jh_coop;

namespace {

constexpr int JH_PAIR_F = 32, JH_SHAPE_F = 16, JH_PAIR_ROWS = 24, JH_ROW_F = 7, JH_PAIR_ROUTINES = 7;

struct PairSink {
  float* rows;  // the pair's own JH_PAIR_ROWS x JH_ROW_F floats
  int n;
  __device__ __forceinline__ void push(const float* pos, const float* nrm, float dist) {
    const int i = n < JH_PAIR_ROWS ? n : JH_PAIR_ROWS - 1;
    float* o = rows + i * JH_ROW_F;
    o[0] = pos[0]; o[1] = pos[1]; o[2] = pos[2]; o[3] = nrm[0]; o[4] = nrm[1]; o[5] = nrm[2]; o[6] = dist;
    n++;
  }
};

__device__ __forceinline__ CvxShape cvx_of(const float* s) {
  CvxShape c{(int)s[0], s[1], s[2], s[3], {s[4], s[5], s[6]}, {}};
  for (int k = 0; k < 9; k++) c.R[k] = s[7 + k];
  return c;
}

__global__ __launch_bounds__(64) void k_collide_pairs(int routine, const float* __restrict__ pairs, int n, float* __restrict__ contacts, int* __restrict__ counts) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  float a[JH_SHAPE_F], b[JH_SHAPE_F];
  for (int k = 0; k < JH_SHAPE_F; k++) { a[k] = pairs[(size_t)i * JH_PAIR_F + k]; b[k] = pairs[(size_t)i * JH_PAIR_F + JH_SHAPE_F + k]; }
  const float *sa = a + 1, *pa = a + 4, *Ra = a + 7, *sb = b + 1, *pb = b + 4, *Rb = b + 7;
  PairSink sk{contacts + (size_t)i * JH_PAIR_ROWS * JH_ROW_F, 0};
  switch (routine) {
    case 0: collide_box_box(sk, pa, Ra, sa, pb, Rb, sb); break;
    case 1: collide_box_sphere(sk, pa, Ra, sa, pb, sb[0]); break;
    case 2: collide_box_capsule(sk, pa, Ra, sa, pb, Rb, sb[0], sb[1]); break;
    case 3: collide_cylinder_sphere(sk, pa, Ra, sa[0], sa[1], pb, sb[0]); break;
    // (one instantiation: the tree kernel's tire build takes the default stop, the leap cylinder build CVX_STOP_NM, and the two are the same 1 000 nm)
    case 4: { const CvxShape A = cvx_of(a), B = cvx_of(b); collide_convex_cylinder<PairSink, CVX_STOP_NM>(sk, A, B); break; }
    case 5: collide_capsule_capsule(sk, pa, Ra, sa[0], sa[1], pb, Rb, sb[0], sb[1]); break;
    default: sk.rows[0] = box_box_distance(pa, Ra, sa, pb, Rb, sb); sk.n = box_box_touching(pa, Ra, sa, pb, Rb, sb) ? 1 : 0; break;
  }
  counts[i] = sk.n;
}

}  // namespace

// routine: 0 box-box, 1 box-sphere, 2 box-capsule, 3 cylinder-sphere, 4 collide_convex_cylinder (GJK + EPA), 5 capsule-capsule,
// 6 box_box_distance + box_box_touching.  `pairs`, `contacts` (n x 24 x 7) and `counts` (n) are device pointers.  Not product interface: bound by tests/pairs.py alone.
extern "C" int jh_xcheck_collide_pairs(int routine, const float* pairs, int n, float* contacts, int* counts, void* stream) {
  JH_REQUIRE(routine >= 0 && routine < JH_PAIR_ROUTINES, "jh_xcheck_collide_pairs: routine %d", routine);
  JH_REQUIRE(pairs && contacts && counts && n >= 0, "jh_xcheck_collide_pairs: null argument or n < 0");
  if (n == 0) return JH_OK;
  hipLaunchKernelGGL(k_collide_pairs, dim3((n + 63) / 64), dim3(64), 0, (hipStream_t)stream, routine, pairs, n, contacts, counts);
  return jh_launch_done(nullptr, (hipStream_t)stream);
}
