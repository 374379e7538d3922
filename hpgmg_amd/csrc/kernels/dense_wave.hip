// dense_wave.hip -- the three streaming passes of the Newmark march of the dense-array solver (include/hpgmg_operators.h hpgmg_wave_predict,
// hpgmg_wave_correct, hpgmg_wave_init).  The cell expressions the host defaults (host/hooks_host.inc) must match bit for bit are not
// written here but in include/hpgmg_wave_math.h, which both compile.
//
//   wave_predict  ut = (u + dt v) + cu q ; vt = v + cv q ; F = F + alpha (a ut - sigma vt) ; u = uold = ut ; v = vt       5 reads, 4 writes: 72 B per cell
//   wave_correct  q = (u - uold) cq ; v = v + cg q ; sum (alpha v) v ; sum u ((F - r) - (a alpha) u)                      6 reads, 2 writes: 64 B per cell
//   wave_init     q = ((r + (a alpha) u) / alpha) - sigma v ; the same two sums                                            5 reads, 1 write:  48 B per cell
//
// One mapping for all three, the CG passes' (pcg_map.hpp): a workgroup of 256 lanes owns 256 consecutive columns of one box over one segment of 16
// planes and marches it in +k, so a lane's two chains over its planes are leaves of the ONE stride-doubling tree of the header; pcg_block_sum2 folds them
// below stride 256 and pcg_fold (pcg.hip) from there upwards, both trees in one launch.  wave_predict has no sum and uses the mapping for its launch
// arithmetic alone.  Ghost and padding doubles are neither read nor written; a NaN or Inf goes into the sums like any value.
#include "pcg_map.hpp"
#include "hpgmg_wave_math.h"

namespace hpgmg {

__global__ __launch_bounds__(kPcgLanes) void wave_predict_kernel(const hpgmg_hip_level L, int u_id, int uold_id, int v_id, int F_id, int q_id, double dt,
                                                                  double cu, double cv, double a, double sigma, int nseg, int ncb, int per_xcd, int items) {
  PcgItem it;
  if (!pcg_item(L, nseg, ncb, per_xcd, items, it) || !it.live) return;
  const int kS = L.kStride, col = it.c % L.dim + (it.c / L.dim) * L.jStride;
  const gptr u = gvec_origin(L, it.box, u_id) + col, uold = gvec_origin(L, it.box, uold_id) + col, v = gvec_origin(L, it.box, v_id) + col;
  const gptr F = gvec_origin(L, it.box, F_id) + col;
  const gcptr q = gvec_origin(L, it.box, q_id) + col, al = gvec_origin(L, it.box, VECTOR_ALPHA) + col;
  for (int k = it.k0; k < it.k1; k++) {
    const int o = k * kS;
    const double uc = u[o], vc = v[o], qc = q[o], Fc = F[o], ac = al[o];
    const double ut = wave_ut_cell(uc, vc, qc, dt, cu), vt = wave_vt_cell(vc, qc, cv);
    F[o] = wave_rhs_cell(Fc, ac, ut, vt, a, sigma);
    u[o] = ut; uold[o] = ut; v[o] = vt;
  }
}

// the workgroups' kinetic values go to partials[item], the potential ones to partials[items + item]: two arrays for the one fold launch
__global__ __launch_bounds__(kPcgLanes) void wave_correct_kernel(const hpgmg_hip_level L, int q_id, int v_id, int u_id, int uold_id, int F_id, int r_id,
                                                                  double a, double cq, double cg, int nseg, int ncb, int per_xcd, int items,
                                                                  double *__restrict__ partials) {
  __shared__ double smem[8];
  PcgItem it;
  if (!pcg_item(L, nseg, ncb, per_xcd, items, it)) return;
  double kin = 0.0, pot = 0.0;
  if (it.live) {
    const int kS = L.kStride, col = it.c % L.dim + (it.c / L.dim) * L.jStride;
    const gptr q = gvec_origin(L, it.box, q_id) + col, v = gvec_origin(L, it.box, v_id) + col;
    const gcptr u = gvec_origin(L, it.box, u_id) + col, uold = gvec_origin(L, it.box, uold_id) + col, F = gvec_origin(L, it.box, F_id) + col;
    const gcptr r = gvec_origin(L, it.box, r_id) + col, al = gvec_origin(L, it.box, VECTOR_ALPHA) + col;
    for (int k = it.k0; k < it.k1; k++) {
      const int o = k * kS;
      const double uc = u[o], uo = uold[o], vc = v[o], Fc = F[o], rc = r[o], ac = al[o];
      const double qn = wave_q_cell(uc, uo, cq), vn = wave_v_cell(vc, qn, cg);
      q[o] = qn; v[o] = vn;
      const double tk = wave_kinetic_cell(ac, vn), tp = wave_potential_cell(uc, Fc, rc, ac, a);
      kin = kin + tk;
      pot = pot + tp;
    }
  }
  pcg_block_sum2(kin, pot, smem);
  if (threadIdx.x == 0) { partials[it.item] = kin; partials[items + it.item] = pot; }
}

__global__ __launch_bounds__(kPcgLanes) void wave_init_kernel(const hpgmg_hip_level L, int q_id, int r_id, int u_id, int v_id, int F_id, double a, double sigma,
                                                               int nseg, int ncb, int per_xcd, int items, double *__restrict__ partials) {
  __shared__ double smem[8];
  PcgItem it;
  if (!pcg_item(L, nseg, ncb, per_xcd, items, it)) return;
  double kin = 0.0, pot = 0.0;
  if (it.live) {
    const int kS = L.kStride, col = it.c % L.dim + (it.c / L.dim) * L.jStride;
    const gptr q = gvec_origin(L, it.box, q_id) + col;
    const gcptr r = gvec_origin(L, it.box, r_id) + col, u = gvec_origin(L, it.box, u_id) + col, v = gvec_origin(L, it.box, v_id) + col;
    const gcptr F = gvec_origin(L, it.box, F_id) + col, al = gvec_origin(L, it.box, VECTOR_ALPHA) + col;
    for (int k = it.k0; k < it.k1; k++) {
      const int o = k * kS;
      const double rc = r[o], uc = u[o], vc = v[o], Fc = F[o], ac = al[o];
      q[o] = wave_init_cell(rc, ac, uc, vc, a, sigma);
      const double tk = wave_kinetic_cell(ac, vc), tp = wave_potential_cell(uc, Fc, rc, ac, a);
      kin = kin + tk;
      pot = pot + tp;
    }
  }
  pcg_block_sum2(kin, pot, smem);
  if (threadIdx.x == 0) { partials[it.item] = kin; partials[items + it.item] = pot; }
}

// the launchers' own refusal: the geometry the mapping holds, and the rule of include/hpgmg_wave_math.h on the ids
static const char *wave_refusal(const hpgmg_hip_level *L, const int *ids, int nout, int n, int num_vectors) {
  if (!pcg_geometry_ok(L) || L->ghosts < 0) return "the level is not one the CG passes' mapping holds";
  if (wave_ids_refused(ids, nout, n, num_vectors, VECTOR_ALPHA)) return "a vector id is outside the level, the level has no alpha, or a vector that is written is named twice";
  return nullptr;
}

}  // namespace hpgmg

using namespace hpgmg;

extern "C" {
int hpgmg_hip_graph_flush(void);

int hpgmg_hip_wave_predict(const hpgmg_hip_level *L, int num_vectors, int u_id, int uold_id, int v_id, int F_id, int q_id, double dt, double cu, double cv,
                           double a, double sigma) {
  const int ids[5] = { u_id, uold_id, v_id, F_id, q_id };
  if (const char *why = wave_refusal(L, ids, 4, 5, num_vectors)) return record_error(hipErrorInvalidValue, why);
  if (int e = hpgmg_hip_graph_flush()) return e;
  const PcgGrid g = pcg_grid(L);
  hipLaunchKernelGGL(wave_predict_kernel, dim3(g.grid), dim3(kPcgLanes), 0, g_stream, *L, u_id, uold_id, v_id, F_id, q_id, dt, cu, cv, a, sigma, g.nseg, g.ncb,
                     g.per_xcd, g.items);
  HPGMG_LAUNCH_CHECK("wave_predict_kernel");
  return 0;
}

int hpgmg_hip_wave_correct(const hpgmg_hip_level *L, int num_vectors, int q_id, int v_id, int u_id, int uold_id, int F_id, int r_id, double a, double cq,
                           double cg, double sums[2]) {
  const int ids[6] = { q_id, v_id, u_id, uold_id, F_id, r_id };
  sums[0] = sums[1] = 0.0;
  if (const char *why = wave_refusal(L, ids, 2, 6, num_vectors)) return record_error(hipErrorInvalidValue, why);
  if (int e = hpgmg_hip_graph_flush()) return e;
  const PcgGrid g = pcg_grid(L);
  double *partials = reduction_scratch(2 * g.items);
  if (!partials) return record_error(hipErrorOutOfMemory, "wave_correct: no scratch");
  hipLaunchKernelGGL(wave_correct_kernel, dim3(g.grid), dim3(kPcgLanes), 0, g_stream, *L, q_id, v_id, u_id, uold_id, F_id, r_id, a, cq, cg, g.nseg, g.ncb,
                     g.per_xcd, g.items, partials);
  HPGMG_LAUNCH_CHECK("wave_correct_kernel");
  return pcg_fold(g.items, &sums[0], &sums[1]);
}

int hpgmg_hip_wave_init(const hpgmg_hip_level *L, int num_vectors, int q_id, int r_id, int u_id, int v_id, int F_id, double a, double sigma, double sums[2]) {
  const int ids[5] = { q_id, r_id, u_id, v_id, F_id };
  sums[0] = sums[1] = 0.0;
  if (const char *why = wave_refusal(L, ids, 1, 5, num_vectors)) return record_error(hipErrorInvalidValue, why);
  if (int e = hpgmg_hip_graph_flush()) return e;
  const PcgGrid g = pcg_grid(L);
  double *partials = reduction_scratch(2 * g.items);
  if (!partials) return record_error(hipErrorOutOfMemory, "wave_init: no scratch");
  hipLaunchKernelGGL(wave_init_kernel, dim3(g.grid), dim3(kPcgLanes), 0, g_stream, *L, q_id, r_id, u_id, v_id, F_id, a, sigma, g.nseg, g.ncb, g.per_xcd, g.items,
                     partials);
  HPGMG_LAUNCH_CHECK("wave_init_kernel");
  return pcg_fold(g.items, &sums[0], &sums[1]);
}

}  // extern "C"
