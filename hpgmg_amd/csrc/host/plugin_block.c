/*
 * plugin_block.c -- hpgmg_block_gram / _combine / _residual of the operator plugin (include/hpgmg_operators.h): one pass of
 * kernels/block.hip each, on the levels the CG passes' kernels take (hp_pcg_backend, plugin_pcg.c).  Anywhere else the portable forms of
 * host/hooks_host.inc run: the same bits, and the return value says which of the two it was.  A refusal (-1) is decided here, before anything is launched.
 */
#include "plugin_internal.h"

/* the portable forms live with the host layer (host/hooks_host.inc); under another driver (INTEGRATION.md Route B) they are absent, and so is every caller */
extern int hpgmg_block_gram_host(level_type *, const int *, int, const int *, int, int, double *) __attribute__((weak));
extern int hpgmg_block_combine_host(level_type *, const int *, int, const int *, int, const double *) __attribute__((weak));
extern int hpgmg_block_residual_host(level_type *, const int *, const int *, const int *, int, int, const double *, double *, double *) __attribute__((weak));
#define PORTABLE(FN, ...) do { if (!FN) hp_no_kernel(#FN " (this level is not one the block kernels take, and the host layer's portable form is not linked)"); return FN(__VA_ARGS__); } while (0)

static backend_t *block_backend(level_type *L) {
  backend_t *B = hp_pcg_backend(L);
  return (B && hpgmg_hip_block_supported(&B->dev)) ? B : NULL;
}
static int block_ids_ok(const level_type *L, const int *ids, int n, int max) {
  int q;
  if (!ids || n < 1 || n > max) return 0;
  for (q = 0; q < n; q++) if (ids[q] < 0 || ids[q] >= L->numVectors) return 0;
  return 1;
}
static int block_ids_distinct(const int *ids, int n) {
  int p, q;
  for (p = 0; p < n; p++) for (q = 0; q < p; q++) if (ids[p] == ids[q]) return 0;
  return 1;
}

int hpgmg_block_gram(level_type *L, const int *a_ids, int na, const int *b_ids, int nb, int w_id, double *G) {
  if (!G || !block_ids_ok(L, a_ids, na, HPGMG_BLOCK_MAX_IN) || !block_ids_ok(L, b_ids, nb, HPGMG_BLOCK_MAX_IN) || w_id >= L->numVectors) return -1;
  backend_t *B = block_backend(L);
  if (!B) PORTABLE(hpgmg_block_gram_host, L, a_ids, na, b_ids, nb, w_id, G);
  BLAS1(hpgmg_hip_block_gram(&B->dev, a_ids, na, b_ids, nb, w_id, G));
  return 1;
}

int hpgmg_block_combine(level_type *L, const int *out_ids, int nout, const int *in_ids, int nin, const double *C) {
  if (!C || !block_ids_ok(L, out_ids, nout, HPGMG_BLOCK_MAX_OUT) || !block_ids_ok(L, in_ids, nin, HPGMG_BLOCK_MAX_IN) || !block_ids_distinct(out_ids, nout)) return -1;
  backend_t *B = block_backend(L);
  if (!B) PORTABLE(hpgmg_block_combine_host, L, out_ids, nout, in_ids, nin, C);
  { int q; for (q = 0; q < nout; q++) hp_coef_written(L, out_ids[q]); }      /* (an output among the coefficient vectors: VECTOR_DINV no longer follows from them) */
  BLAS1(hpgmg_hip_block_combine(&B->dev, out_ids, nout, in_ids, nin, C));
  return 1;
}

int hpgmg_block_residual(level_type *L, const int *r_ids, const int *ax_ids, const int *x_ids, int n, int w_id, const double *mu, double *rmax, double *mxmax) {
  int p, q;
  if (!mu || !rmax || !mxmax || !block_ids_ok(L, r_ids, n, HPGMG_BLOCK_MAX_OUT) || !block_ids_ok(L, ax_ids, n, HPGMG_BLOCK_MAX_OUT) ||
      !block_ids_ok(L, x_ids, n, HPGMG_BLOCK_MAX_OUT) || !block_ids_distinct(r_ids, n) || w_id >= L->numVectors) return -1;
  for (q = 0; q < n; q++) for (p = 0; p < n; p++) if (p != q && (r_ids[q] == ax_ids[p] || r_ids[q] == x_ids[p])) return -1;      /* r_q may alias its own column only */
  if (w_id >= 0) for (q = 0; q < n; q++) if (r_ids[q] == w_id) return -1;
  backend_t *B = block_backend(L);
  if (!B) PORTABLE(hpgmg_block_residual_host, L, r_ids, ax_ids, x_ids, n, w_id, mu, rmax, mxmax);
  for (q = 0; q < n; q++) hp_coef_written(L, r_ids[q]);
  BLAS1(hpgmg_hip_block_residual(&B->dev, r_ids, ax_ids, x_ids, n, w_id, mu, rmax, mxmax));
  return 1;
}
