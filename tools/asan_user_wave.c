/*
 * asan_user_wave.c -- the host defaults of the wave hooks (host/hooks_host.inc hpgmg_wave_predict, _correct, _init) and a small Newmark march
 * (host/user_wave.inc) under AddressSanitizer and UndefinedBehaviorSanitizer: a stand-alone program, no Python and no GPU.
 * It builds a 12^3 level in boxes of 4 from the host layer with the CPU restatement as its plugin, runs the three hooks and their refusals, then a
 * wave_start and three wave_steps (a dt change at the third, a refused step between them) on an 8^3 Helmholtz solver with mixed walls and on a
 * periodic one, and exits 0 if every status and value is what it must be.  tools/asan_user_wave.sh builds and runs it.
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include "hpgmg_fv.h"

#define NV 16
#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "asan_user_wave: line %d: %s\n", __LINE__, #cond); return 1; } } while (0)

static double frand(unsigned *s) { *s = *s * 1664525u + 1013904223u; return (double)(*s >> 8) / 16777216.0; }

static int hooks(int bc) {
  const int n = 12, box = 4, u = VECTOR_U, F = VECTOR_F, r = VECTOR_TEMP, uold = 12, v = 13, q = 14;
  const size_t cells = (size_t)n * n * n;
  const hpgmg_config cfg = { HPGMG_OP_7PT, HPGMG_SMOOTH_CHEBY, 1, 1 };
  unsigned seed = 555u + (unsigned)bc;
  double sums[2], gram;
  int id;
  size_t c;
  CHECK(hpgmg_configure(&cfg) == 0);
  level_type L;
  create_level(&L, n / box, box, stencil_get_radius(), NV, bc, 0, 1);
  L.h = 1.0 / n;
  double *x = (double *)malloc(cells * sizeof(double));
  for (id = 0; id < NV; id++) {
    for (c = 0; c < cells; c++) x[c] = id == VECTOR_ALPHA ? 0.5 + frand(&seed) : frand(&seed) - 0.5;
    CHECK(hpgmg_dense_pack(&L, id, x, HPGMG_WHERE_HOST, HPGMG_DENSE_CELL, HPGMG_DENSE_CHECK_FINITE) == 0);
  }
  CHECK(hpgmg_wave_init(&L, q, r, u, v, F, 3.0e3, 0.2, sums) == 0 && isfinite(sums[0]) && isfinite(sums[1]) && sums[0] > 0.0);
  CHECK(hpgmg_wave_predict(&L, u, uold, v, F, q, 0.03, 1.8e-4, 0.012, 3.0e3, 0.2) == 0);
  CHECK(hpgmg_wave_correct(&L, q, v, u, uold, F, r, 3.0e3, 3.7e3, 0.018, sums) == 0 && isfinite(sums[0]) && isfinite(sums[1]));
  CHECK(hpgmg_block_gram(&L, &v, 1, &v, 1, VECTOR_ALPHA, &gram) == 0 && gram == sums[0]);
  /* refusals */
  CHECK(hpgmg_wave_predict(&L, u, u, v, F, q, 0.03, 0.0, 0.0, 1.0, 0.0) == -1 && hpgmg_wave_predict(&L, u, uold, v, F, NV, 0.03, 0.0, 0.0, 1.0, 0.0) == -1);
  CHECK(hpgmg_wave_correct(&L, q, q, u, uold, F, r, 1.0, 1.0, 1.0, sums) == -1 && hpgmg_wave_correct(&L, VECTOR_ALPHA, v, u, uold, F, r, 1.0, 1.0, 1.0, sums) == -1);
  CHECK(hpgmg_wave_init(&L, u, r, u, v, F, 1.0, 0.0, sums) == -1 && hpgmg_wave_init(&L, q, -1, u, v, F, 1.0, 0.0, sums) == -1);
  CHECK(hpgmg_wave_init(&L, q, r, u, v, F, 1.0, 0.0, NULL) == -1);
  free(x);
  destroy_level(&L);
  return 0;
}

static int march(int periodic, double sigma) {
  const int n = 8;
  const size_t cells = (size_t)n * n * n, big = (size_t)n * n * (n + 1), face = (size_t)6 * n * n;
  const int kinds[6] = { HPGMG_FACE_ROBIN, HPGMG_FACE_DIRICHLET, HPGMG_FACE_NEUMANN, HPGMG_FACE_ROBIN, HPGMG_FACE_DIRICHLET, HPGMG_FACE_NEUMANN };
  unsigned seed = 2424u;
  hpgmg_user_solver *us = NULL;
  hpgmg_user_wave_info info;
  hpgmg_user_info tinfo;
  double rate;
  size_t c;
  int k;
  if (periodic) CHECK(hpgmg_user_create(n, 4, BC_PERIODIC, HPGMG_OP_7PT, HPGMG_SMOOTH_CHEBY, 1.0, 0.7, 0.0, &us) == HPGMG_USER_OK);
  else CHECK(hpgmg_user_create_faces(n, 4, kinds, HPGMG_OP_7PT, HPGMG_SMOOTH_CHEBY, 1.0, 0.7, 0.0, &us) == HPGMG_USER_OK);
  double *alpha = (double *)malloc(cells * sizeof(double)), *beta = (double *)malloc(3 * big * sizeof(double)), *kappa = (double *)malloc(face * sizeof(double));
  double *u = (double *)malloc(4 * cells * sizeof(double)), *v = u + cells, *f = u + 2 * cells, *out = u + 3 * cells, *g = (double *)malloc(face * sizeof(double));
  for (c = 0; c < cells; c++) { alpha[c] = 0.5 + frand(&seed); u[c] = frand(&seed) - 0.5; v[c] = frand(&seed) - 0.5; f[c] = frand(&seed) - 0.5; }
  for (c = 0; c < 3 * big; c++) beta[c] = 0.5 + frand(&seed);
  for (c = 0; c < face; c++) { kappa[c] = frand(&seed); g[c] = frand(&seed) - 0.5; }
  CHECK(hpgmg_user_set_coefficients_robin(us, alpha, beta, beta + big, beta + 2 * big, periodic ? NULL : kappa, HPGMG_WHERE_HOST) == HPGMG_USER_OK);
  CHECK(hpgmg_user_wave_step(us, f, NULL, HPGMG_WHERE_HOST, 0.01, 1e-8, &info) == HPGMG_USER_NOT_READY);
  CHECK(hpgmg_user_wave_start(us, u, v, f, NULL, HPGMG_WHERE_HOST, 0.01, 0.2, 0.5, sigma, &info) == HPGMG_USER_BAD_ARGUMENT);
  CHECK(hpgmg_user_wave_start(us, u, v, f, periodic ? NULL : g, HPGMG_WHERE_HOST, 0.01, 0.25, 0.5, sigma, &info) == HPGMG_USER_OK);
  CHECK(info.t == 0.0 && info.vcycles == 0 && info.kinetic > 0.0 && isfinite(info.potential));
  for (k = 1; k <= 3; k++) {
    const double e0 = info.kinetic + info.potential;
    if (k == 2) {
      f[7] = NAN;
      CHECK(hpgmg_user_wave_step(us, f, periodic ? NULL : g, HPGMG_WHERE_HOST, 0.0, 1e-8, &info) == HPGMG_USER_NOT_FINITE);
      f[7] = 0.25;
    }
    CHECK(hpgmg_user_wave_step(us, f, periodic ? NULL : g, HPGMG_WHERE_HOST, k == 3 ? 0.0025 : 0.0, 1e-8, &info) == HPGMG_USER_OK);
    CHECK(info.converged && info.vcycles > 0 && info.kinetic > 0.0 && isfinite(info.potential) && fabs(info.kinetic + info.potential - e0) < 0.5 * fabs(e0) + 1.0);
    CHECK(hpgmg_user_step(us, f, NULL, HPGMG_WHERE_HOST, 0.01, 1.0, 1e-8, &tinfo, &rate) == HPGMG_USER_NOT_READY);
  }
  CHECK(fabs(info.t - 0.0225) < 1e-15);
  CHECK(hpgmg_user_get_velocity(us, out, HPGMG_WHERE_HOST) == HPGMG_USER_OK && isfinite(out[cells - 1]));
  CHECK(hpgmg_user_get_acceleration(us, out, HPGMG_WHERE_HOST) == HPGMG_USER_OK && isfinite(out[0]));
  CHECK(hpgmg_user_get_rate(us, out, HPGMG_WHERE_HOST) == HPGMG_USER_NOT_READY);
  CHECK(hpgmg_user_start(us, u, f, NULL, HPGMG_WHERE_HOST, 0.01, 1.0) == HPGMG_USER_OK);                      /* a theta march ends the wave march */
  CHECK(hpgmg_user_get_velocity(us, out, HPGMG_WHERE_HOST) == HPGMG_USER_NOT_READY);
  alpha[17] = 0.0;
  CHECK(hpgmg_user_set_coefficients_robin(us, alpha, beta, beta + big, beta + 2 * big, periodic ? NULL : kappa, HPGMG_WHERE_HOST) == HPGMG_USER_OK);
  CHECK(hpgmg_user_wave_start(us, u, v, f, NULL, HPGMG_WHERE_HOST, 0.01, 0.25, 0.5, sigma, &info) == HPGMG_USER_OUT_OF_RANGE);
  free(alpha); free(beta); free(kappa); free(u); free(g);
  hpgmg_user_destroy(us);
  return 0;
}

int main(void) {
  hpgmg_verbose = 0;
  if (hooks(BC_DIRICHLET) || hooks(BC_PERIODIC) || march(0, 0.3) || march(1, 0.0)) return 1;
  printf("asan_user_wave: clean\n");
  return 0;
}
