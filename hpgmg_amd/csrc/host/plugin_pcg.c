/*
 * plugin_pcg.c -- hpgmg_pcg_apply_dot / _update / _dot / _dot2 of the operator plugin (include/hpgmg_operators.h): one pass of
 * kernels/pcg.hip each, on the levels those kernels take -- the 7-point variable-coefficient operator in ghost-free mode with every box local, which
 * is every level of a user problem.  Anywhere else the portable forms of host/hooks_host.inc run (the operators, then the sums on the host): the same bits,
 * and the return value says which of the two it was.
 */
#include "plugin_internal.h"

/* the portable forms live with the host layer (host/hooks_host.inc); under another driver (INTEGRATION.md Route B) they are absent, and so is every caller */
extern int hpgmg_pcg_apply_dot_host(level_type *, int, int, double, double, double *) __attribute__((weak));
extern int hpgmg_pcg_update_host(level_type *, int, int, int, int, double, double *) __attribute__((weak));
extern int hpgmg_pcg_dot_host(level_type *, int, int, double *) __attribute__((weak));
extern int hpgmg_pcg_dot2_host(level_type *, int, int, int, double *, double *) __attribute__((weak));
#define PORTABLE(FN, ...) do { if (!FN) hp_no_kernel(#FN " (this level is not one the CG kernels take, and the host layer's portable form is not linked)"); return FN(__VA_ARGS__); } while (0)

backend_t *hp_pcg_backend(level_type *L) {      /* the levels the CG passes' kernels take (host/plugin_block.c asks too); NULL: the portable forms */
  hpgmg_config c;
  hpgmg_get_config(&c);
  if (c.op != HPGMG_OP_7PT || !c.variable_coeff || !hp_ghost_free_mode() || !L->active || L->num_my_boxes < 1 || L->num_ranks != 1) return NULL;
  backend_t *B = hp_backend_of(L);
  if (!B->all_faces_local || !hpgmg_hip_pcg_supported(&B->dev, hp_variant())) return NULL;
  return B;
}
static int pcg_ids_ok(const level_type *L, int a, int b, int c, int d) {
  return a >= 0 && a < L->numVectors && b >= 0 && b < L->numVectors && c >= 0 && c < L->numVectors && d >= 0 && d < L->numVectors;
}

int hpgmg_pcg_apply_dot(level_type *L, int Ap_id, int p_id, double a, double b, double *dot) {
  backend_t *B = hp_pcg_backend(L);
  double v = 0.0;
  if (!B || Ap_id == p_id || !pcg_ids_ok(L, Ap_id, p_id, 0, 0)) PORTABLE(hpgmg_pcg_apply_dot_host, L, Ap_id, p_id, a, b, dot);
  { TICK(L, apply_op, "apply_op + dot (fused)");
    HIP_OK(hpgmg_hip_pcg_apply_dot(&B->dev, hp_variant(), Ap_id, p_id, a, b, 1.0 / (L->h * L->h), &v));
    TOCK(); }
  *dot = hp_allreduce_scalar(L, v, HPGMG_REDUCE_SUM);
  return 1;
}

int hpgmg_pcg_update(level_type *L, int x_id, int r_id, int p_id, int Ap_id, double alpha, double *rmax) {
  backend_t *B = hp_pcg_backend(L);
  double v = 0.0;
  if (!B || x_id == r_id || x_id == p_id || x_id == Ap_id || r_id == p_id || r_id == Ap_id || !pcg_ids_ok(L, x_id, r_id, p_id, Ap_id))
    PORTABLE(hpgmg_pcg_update_host, L, x_id, r_id, p_id, Ap_id, alpha, rmax);
  BLAS1(hpgmg_hip_pcg_update(&B->dev, x_id, r_id, p_id, Ap_id, alpha, &v));
  *rmax = hp_allreduce_scalar(L, v, HPGMG_REDUCE_MAX);
  return 1;
}

int hpgmg_pcg_dot(level_type *L, int a_id, int b_id, double *dot) {
  backend_t *B = hp_pcg_backend(L);
  double v = 0.0;
  if (!B || !pcg_ids_ok(L, a_id, b_id, 0, 0)) PORTABLE(hpgmg_pcg_dot_host, L, a_id, b_id, dot);
  BLAS1(hpgmg_hip_pcg_dot(&B->dev, a_id, b_id, &v));
  *dot = hp_allreduce_scalar(L, v, HPGMG_REDUCE_SUM);
  return 1;
}

int hpgmg_pcg_dot2(level_type *L, int a_id, int c_id, int b_id, double *ab, double *cb) {
  backend_t *B = hp_pcg_backend(L);
  double v = 0.0, w = 0.0;
  if (!B || !pcg_ids_ok(L, a_id, c_id, b_id, 0)) PORTABLE(hpgmg_pcg_dot2_host, L, a_id, c_id, b_id, ab, cb);
  BLAS1(hpgmg_hip_pcg_dot2(&B->dev, a_id, c_id, b_id, &v, &w));
  *ab = hp_allreduce_scalar(L, v, HPGMG_REDUCE_SUM);
  *cb = hp_allreduce_scalar(L, w, HPGMG_REDUCE_SUM);
  return 1;
}
