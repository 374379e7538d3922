/*
 * plugin_step.c -- hpgmg_step_rhs / hpgmg_step_rate of the operator plugin (include/hpgmg_operators.h): one launch of
 * kernels/dense_step.hip each, over the level's boxes where they live.  They replace the weak host defaults of host/hooks_host.inc, which go
 * box by box through hpgmg_vector_upload / download.  A level or vector ids the kernels refuse stop the program, as every failed launch does.
 */
#include "plugin_internal.h"

void hpgmg_step_rhs(level_type *L, int F_id, int u_id, int uold_id, int w_id, double a, double c) {
  backend_t *B = hp_backend_of(L);
  hp_coef_written(L, F_id); hp_coef_written(L, uold_id);
  BLAS1(hpgmg_hip_step_rhs(&B->dev, L->numVectors, F_id, u_id, uold_id, w_id, a, c));
}

void hpgmg_step_rate(level_type *L, int w_id, int r_id, int u_id, int uold_id, double a, double c, double *max_abs) {
  backend_t *B = hp_backend_of(L);
  double v = 0.0;
  hp_coef_written(L, w_id);
  BLAS1(hpgmg_hip_step_rate(&B->dev, L->numVectors, w_id, r_id, u_id, uold_id, a, c, &v));
  *max_abs = hp_allreduce_scalar(L, v, HPGMG_REDUCE_MAX);
}
