/*
 * hpgmg_step_math.h -- INTERNAL: the two cell expressions of the implicit time march of the dense-array solver (include/hpgmg_operators.h
 * hpgmg_step_rhs, hpgmg_step_rate), written once for the host defaults (host/hooks_host.inc) and the kernels
 * (kernels/dense_step.hip).  Not part of the C ABI, like hpgmg_boundary_math.h: every build has -ffp-contract=off, so the written order of each
 * expression IS the contract between the two.  Compiles as gnu99 C and as HIP C++.
 */
#ifndef HPGMG_STEP_MATH_H
#define HPGMG_STEP_MATH_H

#ifdef __HIPCC__
#define HPGMG_STEP_FN __host__ __device__ __forceinline__
#else
#define HPGMG_STEP_FN static inline
#endif

/* the right-hand side of one theta step, F = f + T(g) on entry:  F + (a alpha u + c w),  a = 1 / (theta dt), c = (1 - theta) / theta */
HPGMG_STEP_FN double step_rhs_cell(double F, double alpha, double u, double w, double a, double c) { return F + ((a * alpha) * u + c * w); }
/* the new rate from the residual r = F - A u of that step's solve:  (r + a alpha (u - u_old)) - c w */
HPGMG_STEP_FN double step_rate_cell(double r, double alpha, double u, double u_old, double w, double a, double c) {
  return (r + (a * alpha) * (u - u_old)) - c * w;
}

#endif
