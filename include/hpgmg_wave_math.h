/*
 * hpgmg_wave_math.h -- INTERNAL: the cell expressions of the Newmark march of the dense-array solver (include/hpgmg_operators.h hpgmg_wave_predict,
 * hpgmg_wave_correct, hpgmg_wave_init), written once for the host defaults (host/hooks_host.inc) and the kernels
 * (kernels/dense_wave.hip), and the one rule by which all three layers refuse a call.  Not part of the C ABI, like hpgmg_step_math.h: every build has
 * -ffp-contract=off, so the written order of each expression IS the contract between the two.  Compiles as gnu99 C and as HIP C++.
 */
#ifndef HPGMG_WAVE_MATH_H
#define HPGMG_WAVE_MATH_H

#ifdef __HIPCC__
#define HPGMG_WAVE_FN __host__ __device__ __forceinline__
#else
#define HPGMG_WAVE_FN static inline
#endif

/* the predictor:  ut = (u + dt v) + cu q,  vt = v + cv q,  cu = dt^2 (1/2 - beta), cv = dt (1 - gamma) */
HPGMG_WAVE_FN double wave_ut_cell(double u, double v, double q, double dt, double cu) { return (u + dt * v) + cu * q; }
HPGMG_WAVE_FN double wave_vt_cell(double v, double q, double cv) { return v + cv * q; }
/* the right-hand side of the step's solve, F = f + T(g) on entry:  F + alpha (a ut - sigma vt) */
HPGMG_WAVE_FN double wave_rhs_cell(double F, double alpha, double ut, double vt, double a, double sigma) { return F + alpha * (a * ut - sigma * vt); }
/* the corrector:  q = (u - ut) cq,  v = vt + cg q,  cq = 1 / (beta dt^2), cg = gamma dt */
HPGMG_WAVE_FN double wave_q_cell(double u, double ut, double cq) { return (u - ut) * cq; }
HPGMG_WAVE_FN double wave_v_cell(double vt, double q, double cg) { return vt + cg * q; }
/* the acceleration at the start from the residual r = F - A0 u:  ((r + (a alpha) u) / alpha) - sigma v */
HPGMG_WAVE_FN double wave_init_cell(double r, double alpha, double u, double v, double a, double sigma) { return ((r + (a * alpha) * u) / alpha) - sigma * v; }
/* the leaf terms of the two sums: the kinetic one is hpgmg_block_gram's weighted (w a) b, the potential one u (K u) with K u = (F - r) - (a alpha) u */
HPGMG_WAVE_FN double wave_kinetic_cell(double alpha, double v) { return (alpha * v) * v; }
HPGMG_WAVE_FN double wave_potential_cell(double u, double F, double r, double alpha, double a) { return u * ((F - r) - (a * alpha) * u); }

/* 1: the call is refused.  ids[0 .. nout) are written, ids[nout .. n) only read; alpha_id is read.  Every id names a vector of the level, the level has an
 * alpha, and no vector that is written is any other vector of the call or alpha (a cell's own reads come before its writes: that is all the aliasing
 * the passes have, and it is written into their signatures). */
HPGMG_WAVE_FN int wave_ids_refused(const int *ids, int nout, int n, int num_vectors, int alpha_id) {
  int p, q;
  if (num_vectors <= alpha_id) return 1;
  for (q = 0; q < n; q++) if (ids[q] < 0 || ids[q] >= num_vectors) return 1;
  for (q = 0; q < nout; q++) {
    if (ids[q] == alpha_id) return 1;
    for (p = 0; p < n; p++) if (p != q && ids[p] == ids[q]) return 1;
  }
  return 0;
}

#endif
