/*
 * asan_user_eigs.c -- the host defaults of the block hooks (host/hooks_host.inc hpgmg_block_gram, _combine, _residual) and one small hpgmg_user_eigs
 * (host/user_eigs.inc) under AddressSanitizer and UndefinedBehaviorSanitizer: a stand-alone program, no Python and no GPU.
 * It builds a 12^3 level in boxes of 4 with 48 vectors from the host layer with the CPU restatement as its plugin, runs the three hooks at the list
 * sizes on the edges of the 6 x 6 pair tile (1, 5, 6, 7, 13, 36; 12 outputs), with aliased outputs and the refusals, then eigs on an 8^3 Helmholtz
 * solver with mixed walls and on a Poisson one, and exits 0 if every status and value is what it must be.  tools/asan_user_eigs.sh builds and runs it.
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include "hpgmg_fv.h"

#define NV 48
#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "asan_user_eigs: line %d: %s\n", __LINE__, #cond); return 1; } } while (0)

static double frand(unsigned *s) { *s = *s * 1664525u + 1013904223u; return (double)(*s >> 8) / 16777216.0; }

static int hooks(int bc) {
  static const int sizes[6] = { 1, 5, 6, 7, 13, 36 };
  const int n = 12, box = 4;
  const size_t cells = (size_t)n * n * n;
  const hpgmg_config cfg = { HPGMG_OP_7PT, HPGMG_SMOOTH_CHEBY, 1, 1 };
  unsigned seed = 777u + (unsigned)bc;
  int ids[NV], v, p, q, i, j;
  size_t c;
  CHECK(hpgmg_configure(&cfg) == 0);
  level_type L;
  create_level(&L, n / box, box, stencil_get_radius(), NV, bc, 0, 1);
  L.h = 1.0 / n;
  double *x = (double *)malloc(cells * sizeof(double));
  for (v = 0; v < NV; v++) {
    for (c = 0; c < cells; c++) x[c] = v ? frand(&seed) - 0.5 : 0.5 + frand(&seed);      /* vector 0: the weight */
    CHECK(hpgmg_dense_pack(&L, v, x, HPGMG_WHERE_HOST, HPGMG_DENSE_CELL, HPGMG_DENSE_CHECK_FINITE) == 0);
    ids[v] = v;
  }
  double *G = (double *)malloc(36 * 36 * sizeof(double)), *C = (double *)malloc(36 * 12 * sizeof(double));
  double mu[12], rmax[12], mxmax[12], one;
  for (p = 0; p < 6; p++) for (q = 0; q < 6; q++) {
    const int na = sizes[p], nb = sizes[q], w = (p + q) & 1 ? 0 : -1;
    CHECK(hpgmg_block_gram(&L, ids + 1, na, ids + 1 + (p == q ? 0 : 11), nb, w, G) == 0);
    for (i = 0; i < na * nb; i++) CHECK(isfinite(G[i]));
    if (p == q) for (i = 0; i < na; i++) for (j = 0; j < i; j++) CHECK(G[i * nb + j] == G[j * nb + i]);
    if (w < 0) { CHECK(hpgmg_pcg_dot(&L, ids[na], ids[nb + (p == q ? 0 : 11)], &one) == 0); CHECK(one == G[(na - 1) * nb + nb - 1]); }
  }
  for (p = 0; p < 6; p++) {
    const int nin = sizes[p], nout = nin < 12 ? nin : 12;
    for (i = 0; i < nin * nout; i++) C[i] = frand(&seed) - 0.5;
    CHECK(hpgmg_block_combine(&L, ids + 1, nout, ids + 1, nin, C) == 0);              /* the outputs are the first inputs */
    CHECK(hpgmg_block_combine(&L, ids + 36, 12, ids + 1, nin, C) == 0);              /* 12 outputs, none an input while nin < 36 */
    CHECK(hpgmg_block_combine(&L, ids + 47, 1, ids + 1, nin, C) == 0);
  }
  for (q = 0; q < 12; q++) mu[q] = 0.5 + q;
  CHECK(hpgmg_block_residual(&L, ids + 25, ids + 1, ids + 13, 12, 0, mu, rmax, mxmax) == 0);
  CHECK(hpgmg_block_residual(&L, ids + 25, ids + 1, ids + 13, 1, -1, mu, rmax, mxmax) == 0);
  CHECK(isfinite(rmax[0]) && mxmax[0] > 0.0);
  /* refusals */
  { int twice[3] = { 40, 41, 40 }, beyond[1] = { NV };
    CHECK(hpgmg_block_combine(&L, twice, 3, ids + 1, 4, C) == -1);
    CHECK(hpgmg_block_combine(&L, ids + 1, 13, ids + 1, 4, C) == -1 && hpgmg_block_combine(&L, ids + 1, 1, ids + 1, 37, C) == -1);
    CHECK(hpgmg_block_combine(&L, beyond, 1, ids + 1, 4, C) == -1 && hpgmg_block_gram(&L, beyond, 1, ids + 1, 4, -1, G) == -1);
    CHECK(hpgmg_block_gram(&L, ids + 1, 37, ids + 1, 1, -1, G) == -1 && hpgmg_block_gram(&L, ids + 1, 0, ids + 1, 1, -1, G) == -1);
    CHECK(hpgmg_block_residual(&L, twice, ids + 1, ids + 13, 3, -1, mu, rmax, mxmax) == -1);
    CHECK(hpgmg_block_residual(&L, ids + 2, ids + 1, ids + 13, 2, -1, mu, rmax, mxmax) == -1); }      /* r_0 is ax_1 */
  free(x); free(G); free(C);
  destroy_level(&L);
  return 0;
}

static int eigs(double a, int robin) {
  const int n = 8, k = 3, extra = 2;
  const size_t cells = (size_t)n * n * n, big = (size_t)n * n * (n + 1), face = (size_t)6 * n * n;
  const int kinds[6] = { HPGMG_FACE_ROBIN, HPGMG_FACE_DIRICHLET, HPGMG_FACE_NEUMANN, HPGMG_FACE_ROBIN, HPGMG_FACE_DIRICHLET, HPGMG_FACE_NEUMANN };
  unsigned seed = 4242u;
  hpgmg_user_solver *us = NULL;
  hpgmg_user_eig_info info;
  size_t c;
  int j;
  if (robin) CHECK(hpgmg_user_create_faces(n, 4, kinds, HPGMG_OP_7PT, HPGMG_SMOOTH_CHEBY, a, 0.7, 0.0, &us) == HPGMG_USER_OK);
  else CHECK(hpgmg_user_create(n, 4, BC_DIRICHLET, HPGMG_OP_7PT, HPGMG_SMOOTH_CHEBY, a, 0.7, 0.0, &us) == HPGMG_USER_OK);
  double *alpha = (double *)malloc(cells * sizeof(double)), *beta = (double *)malloc(3 * big * sizeof(double)), *kappa = (double *)malloc(face * sizeof(double));
  double *modes = (double *)malloc((size_t)(k + extra) * cells * sizeof(double)), lam[12];
  for (c = 0; c < cells; c++) alpha[c] = 0.5 + frand(&seed);
  for (c = 0; c < 3 * big; c++) beta[c] = 0.5 + frand(&seed);
  for (c = 0; c < face; c++) kappa[c] = frand(&seed);
  CHECK(hpgmg_user_set_coefficients_robin(us, a != 0.0 ? alpha : NULL, beta, beta + big, beta + 2 * big, robin ? kappa : NULL, HPGMG_WHERE_HOST) == HPGMG_USER_OK);
  CHECK(hpgmg_user_eigs(us, k, extra, 1e-6, 60, NULL, HPGMG_WHERE_HOST, lam, modes, &info) == HPGMG_USER_OK);
  CHECK(info.converged && info.iterations > 0 && info.iterations <= 60 && lam[0] > 0.0 && lam[0] <= lam[1] && lam[1] <= lam[2]);
  for (j = 0; j < k; j++) CHECK(info.residuals[j] < 1e-6 && fabs(info.mu[j] - (lam[j] + a)) <= 1e-12 * info.mu[j]);
  /* the returned block as the start of a larger one (12 columns: the widest S), and the refusals */
  for (c = (size_t)k * cells; c < (size_t)(k + extra) * cells; c++) modes[c] = frand(&seed) - 0.5;
  CHECK(hpgmg_user_eigs(us, k, extra, 1e-6, 60, modes, HPGMG_WHERE_HOST, lam, modes, &info) == HPGMG_USER_OK && info.converged && info.iterations <= 1);
  CHECK(hpgmg_user_eigs(us, 10, 2, 1e-3, 4, NULL, HPGMG_WHERE_HOST, lam, NULL, &info) == HPGMG_USER_BAD_ARGUMENT);
  { double *wide = (double *)malloc(10 * cells * sizeof(double));
    CHECK(hpgmg_user_eigs(us, 10, 2, 1e-3, 4, NULL, HPGMG_WHERE_HOST, lam, wide, &info) == HPGMG_USER_OK && info.iterations <= 4);
    free(wide); }
  CHECK(hpgmg_user_eigs(us, 0, 2, 1e-6, 60, NULL, HPGMG_WHERE_HOST, lam, modes, &info) == HPGMG_USER_BAD_ARGUMENT);
  CHECK(hpgmg_user_eigs(us, 11, 2, 1e-6, 60, NULL, HPGMG_WHERE_HOST, lam, modes, &info) == HPGMG_USER_BAD_ARGUMENT);
  modes[5] = NAN;
  CHECK(hpgmg_user_eigs(us, k, extra, 1e-6, 60, modes, HPGMG_WHERE_HOST, lam, modes, &info) == HPGMG_USER_NOT_FINITE);
  if (a != 0.0) {
    alpha[17] = 0.0;
    CHECK(hpgmg_user_set_coefficients_robin(us, alpha, beta, beta + big, beta + 2 * big, robin ? kappa : NULL, HPGMG_WHERE_HOST) == HPGMG_USER_OK);
    CHECK(hpgmg_user_eigs(us, k, extra, 1e-6, 60, NULL, HPGMG_WHERE_HOST, lam, modes, &info) == HPGMG_USER_OUT_OF_RANGE);
  }
  free(alpha); free(beta); free(kappa); free(modes);
  hpgmg_user_destroy(us);
  return 0;
}

int main(void) {
  hpgmg_verbose = 0;
  if (hooks(BC_DIRICHLET) || hooks(BC_PERIODIC) || eigs(1.3, 1) || eigs(0.0, 0)) return 1;
  printf("asan_user_eigs: clean\n");
  return 0;
}
