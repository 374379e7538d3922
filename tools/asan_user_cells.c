/*
 * asan_user_cells.c -- the host defaults of the cell-centred conductivity hooks (host/hooks_host.inc hpgmg_dense_pack_cell_mean,
 * hpgmg_dense_unpack_cell_sensitivity) under AddressSanitizer and UndefinedBehaviorSanitizer: a stand-alone program, no
 * Python and no GPU.  It builds a 12^3 level in boxes of 4 from the host layer with the CPU restatement as its plugin, calls the two hooks with a
 * mixed wall mask (and kappa), with both means, on a periodic level without a mask and with an array the hooks must report, and exits 0 if every
 * status and every output entry is what it must be.  tools/asan_user_cells.sh builds and runs it.
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include "hpgmg_fv.h"

#define MIXED 0x1a                    /* i-high, j-high and k-low are masked walls; the other three Dirichlet */
#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "asan_user_cells: line %d: %s\n", __LINE__, #cond); return 1; } } while (0)

static double frand(unsigned *s) { *s = *s * 1664525u + 1013904223u; return (double)(*s >> 8) / 16777216.0; }

static int run(int bc, int mask) {
  const int n = 12, box = 4;
  const size_t cells = (size_t)n * n * n, face = (size_t)6 * n * n;
  const hpgmg_config cfg = { HPGMG_OP_7PT, HPGMG_SMOOTH_CHEBY, 1, 1 };
  unsigned seed = 12345u + (unsigned)mask;
  size_t q;
  int mean;
  CHECK(hpgmg_configure(&cfg) == 0);
  level_type L;
  create_level(&L, n / box, box, stencil_get_radius(), hpgmg_vectors_reserved(), bc, 0, 1);
  L.h = 1.0 / n;
  double *k = (double *)malloc(cells * sizeof(double)), *u = (double *)malloc(cells * sizeof(double)), *lam = (double *)malloc(cells * sizeof(double));
  double *d_alpha = (double *)malloc(cells * sizeof(double)), *d_k = (double *)malloc(cells * sizeof(double)), *host = (double *)malloc(face * sizeof(double));
  for (q = 0; q < cells; q++) { k[q] = 0.5 + frand(&seed); u[q] = frand(&seed) - 0.5; lam[q] = frand(&seed) - 0.5; }
  double *wall = hpgmg_vector_alloc(face), *g = hpgmg_vector_alloc(face), *kappa = hpgmg_vector_alloc(face);
  for (q = 0; q < face; q++) host[q] = frand(&seed) * 2.0;
  hpgmg_vector_upload(g, host, face);
  hpgmg_vector_upload(kappa, host, face);
  CHECK(hpgmg_dense_pack(&L, VECTOR_U, u, HPGMG_WHERE_HOST, HPGMG_DENSE_CELL, HPGMG_DENSE_CHECK_FINITE) == 0);
  CHECK(hpgmg_dense_pack(&L, VECTOR_F, lam, HPGMG_WHERE_HOST, HPGMG_DENSE_CELL, HPGMG_DENSE_CHECK_FINITE) == 0);
  exchange_boundary(&L, VECTOR_U, stencil_get_shape());
  exchange_boundary(&L, VECTOR_F, stencil_get_shape());
  for (mean = HPGMG_MEAN_HARMONIC; mean <= HPGMG_MEAN_ARITHMETIC; mean++) {
    CHECK(hpgmg_dense_pack_cell_mean(&L, k, HPGMG_WHERE_HOST, mean, mask, mask ? wall : NULL) == 0);
    for (q = 0; q < cells; q++) d_alpha[q] = d_k[q] = NAN;
    CHECK(hpgmg_dense_unpack_cell_sensitivity(&L, VECTOR_U, VECTOR_F, k, mean, bc == BC_DIRICHLET ? g : NULL, 1.3, 0.7, mask, mask ? wall : NULL,
                                              mask ? kappa : NULL, d_alpha, d_k, HPGMG_WHERE_HOST) == 0);
    for (q = 0; q < cells; q++) CHECK(isfinite(d_alpha[q]) && isfinite(d_k[q]));
  }
  if (mask) {                         /* the masked walls' betas are the wall cells' own values: face 1 (i-high) entry [k][j] is cell (n - 1, j, k) */
    hpgmg_vector_download(host, wall, face);
    for (q = 0; q < (size_t)n * n; q++) CHECK(host[(size_t)n * n + q] == k[q * n + (n - 1)]);
  }
  /* what the hooks must report: the first and the last entry, and two neighbours whose product overflows */
  k[0] = NAN;
  CHECK(hpgmg_dense_pack_cell_mean(&L, k, HPGMG_WHERE_HOST, HPGMG_MEAN_HARMONIC, mask, mask ? wall : NULL) == HPGMG_DENSE_NOT_FINITE);
  k[0] = 1.0; k[cells - 1] = -1.0;
  CHECK(hpgmg_dense_pack_cell_mean(&L, k, HPGMG_WHERE_HOST, HPGMG_MEAN_HARMONIC, mask, mask ? wall : NULL) == HPGMG_DENSE_OUT_OF_RANGE);
  CHECK(hpgmg_dense_unpack_cell_sensitivity(&L, VECTOR_U, VECTOR_F, k, HPGMG_MEAN_ARITHMETIC, NULL, 1.3, 0.7, mask, mask ? wall : NULL, NULL, NULL, d_k,
                                            HPGMG_WHERE_HOST) == HPGMG_DENSE_OUT_OF_RANGE);
  k[cells - 1] = 1.0; k[700] = k[701] = 1e200;
  CHECK(hpgmg_dense_pack_cell_mean(&L, k, HPGMG_WHERE_HOST, HPGMG_MEAN_HARMONIC, mask, mask ? wall : NULL) == HPGMG_DENSE_NOT_FINITE);
  CHECK(hpgmg_dense_pack_cell_mean(&L, k, HPGMG_WHERE_HOST, HPGMG_MEAN_ARITHMETIC, mask, mask ? wall : NULL) == 0);
  /* refusals */
  CHECK(hpgmg_dense_pack_cell_mean(&L, NULL, HPGMG_WHERE_HOST, HPGMG_MEAN_HARMONIC, 0, NULL) == -1);
  CHECK(hpgmg_dense_pack_cell_mean(&L, k, HPGMG_WHERE_HOST, 2, 0, NULL) == -1);
  CHECK(hpgmg_dense_pack_cell_mean(&L, k, HPGMG_WHERE_HOST, HPGMG_MEAN_HARMONIC, 64, wall) == -1);
  CHECK(hpgmg_dense_pack_cell_mean(&L, k, HPGMG_WHERE_HOST, HPGMG_MEAN_HARMONIC, 5, NULL) == -1);
  if (bc == BC_PERIODIC) CHECK(hpgmg_dense_pack_cell_mean(&L, k, HPGMG_WHERE_HOST, HPGMG_MEAN_HARMONIC, 5, wall) == -1);
  CHECK(hpgmg_dense_unpack_cell_sensitivity(&L, VECTOR_U, VECTOR_F, k, HPGMG_MEAN_HARMONIC, NULL, 1.3, 0.7, 0, NULL, NULL, NULL, NULL, HPGMG_WHERE_HOST) == -1);
  hpgmg_vector_free(wall); hpgmg_vector_free(g); hpgmg_vector_free(kappa);
  free(k); free(u); free(lam); free(d_alpha); free(d_k); free(host);
  destroy_level(&L);
  return 0;
}

int main(void) {
  hpgmg_verbose = 0;
  if (run(BC_DIRICHLET, MIXED) || run(BC_DIRICHLET, 0) || run(BC_DIRICHLET, 63) || run(BC_PERIODIC, 0)) return 1;
  printf("asan_user_cells: clean\n");
  return 0;
}
