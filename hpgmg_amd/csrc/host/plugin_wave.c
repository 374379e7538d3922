/*
 * plugin_wave.c -- hpgmg_wave_predict / _correct / _init of the operator plugin (include/hpgmg_operators.h): one pass of
 * kernels/dense_wave.hip each, on the Helmholtz levels the CG passes' kernels take (hp_pcg_backend, plugin_pcg.c).  Anywhere else the portable forms of
 * host/hooks_host.inc run: the same bits, and the return value says which of the two it was.  A refusal (-1) is decided here, by the rule of
 * include/hpgmg_wave_math.h, before anything is launched.  The sums are the rank's own, as hpgmg_block_gram's (the kernels take one-rank levels only).
 */
#include "plugin_internal.h"
#include "hpgmg_wave_math.h"

/* the portable forms live with the host layer (host/hooks_host.inc); under another driver (INTEGRATION.md Route B) they are absent, and so is every caller */
extern int hpgmg_wave_predict_host(level_type *, int, int, int, int, int, double, double, double, double, double) __attribute__((weak));
extern int hpgmg_wave_correct_host(level_type *, int, int, int, int, int, int, double, double, double, double[2]) __attribute__((weak));
extern int hpgmg_wave_init_host(level_type *, int, int, int, int, int, double, double, double[2]) __attribute__((weak));
#define PORTABLE(FN, ...) do { if (!FN) hp_no_kernel(#FN " (this level is not one the wave kernels take, and the host layer's portable form is not linked)"); return FN(__VA_ARGS__); } while (0)

static backend_t *wave_backend(level_type *L) {
  backend_t *B = hp_pcg_backend(L);
  return (B && hp_variant() == HPGMG_HIP_7PT_VC_HELMHOLTZ) ? B : NULL;
}

int hpgmg_wave_predict(level_type *L, int u_id, int uold_id, int v_id, int F_id, int q_id, double dt, double cu, double cv, double a, double sigma) {
  const int ids[5] = { u_id, uold_id, v_id, F_id, q_id };
  int q;
  if (wave_ids_refused(ids, 4, 5, L->numVectors, VECTOR_ALPHA)) return -1;
  backend_t *B = wave_backend(L);
  if (!B) PORTABLE(hpgmg_wave_predict_host, L, u_id, uold_id, v_id, F_id, q_id, dt, cu, cv, a, sigma);
  for (q = 0; q < 4; q++) hp_coef_written(L, ids[q]);
  BLAS1(hpgmg_hip_wave_predict(&B->dev, L->numVectors, u_id, uold_id, v_id, F_id, q_id, dt, cu, cv, a, sigma));
  return 1;
}

int hpgmg_wave_correct(level_type *L, int q_id, int v_id, int u_id, int uold_id, int F_id, int r_id, double a, double cq, double cg, double sums[2]) {
  const int ids[6] = { q_id, v_id, u_id, uold_id, F_id, r_id };
  if (!sums || wave_ids_refused(ids, 2, 6, L->numVectors, VECTOR_ALPHA)) return -1;
  backend_t *B = wave_backend(L);
  if (!B) PORTABLE(hpgmg_wave_correct_host, L, q_id, v_id, u_id, uold_id, F_id, r_id, a, cq, cg, sums);
  hp_coef_written(L, q_id); hp_coef_written(L, v_id);
  BLAS1(hpgmg_hip_wave_correct(&B->dev, L->numVectors, q_id, v_id, u_id, uold_id, F_id, r_id, a, cq, cg, sums));
  return 1;
}

int hpgmg_wave_init(level_type *L, int q_id, int r_id, int u_id, int v_id, int F_id, double a, double sigma, double sums[2]) {
  const int ids[5] = { q_id, r_id, u_id, v_id, F_id };
  if (!sums || wave_ids_refused(ids, 1, 5, L->numVectors, VECTOR_ALPHA)) return -1;
  backend_t *B = wave_backend(L);
  if (!B) PORTABLE(hpgmg_wave_init_host, L, q_id, r_id, u_id, v_id, F_id, a, sigma, sums);
  hp_coef_written(L, q_id);
  BLAS1(hpgmg_hip_wave_init(&B->dev, L->numVectors, q_id, r_id, u_id, v_id, F_id, a, sigma, sums));
  return 1;
}
