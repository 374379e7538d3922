/*
 * driver.c -- problem setup, the benchmark protocol and the C-ABI accessors.
 *
 * Behavioural reference: finite-volume/source/hpgmg-fv.c
 *   bench_hpgmg :50-99 (warm-up solves, then timed solves, zero_vector(U) first)
 *   main :103-386 (argument rules :152-205, setup :283-308, the h/2h/4h loop
 *   :320-345 with its "DOF/s" line :344, Richardson analysis :351-366)
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>
#include <math.h>
#include <stdint.h>
#include "hpgmg_fv.h"
#ifdef _OPENMP
#include <omp.h>
#endif
/* OpenMP threads of the host build (hpgmg-fv.c:137-147 prints omp_get_max_threads()); the HIP build has one host thread */
static int host_threads(void) {
#ifdef _OPENMP
  if (strcmp(hpgmg_backend_name(), "hip") != 0) return omp_get_max_threads();
#endif
  return 1;
}

/* CPU threads this process may really use: a container reports every core of the machine (256 on the GPU boxes) but is
 * scheduled on a cgroup quota (16 there); an OpenMP team of 256 spinning threads on 16 CPUs makes every parallel
 * region crawl.  Unless the user set OMP_NUM_THREADS, cap the team at min(quota, affinity mask) when the library loads. */
int hpgmg_usable_cpus(void) {
  long n = -1;
#ifdef _OPENMP
  n = omp_get_num_procs();
#endif
  if (n < 1) n = 1;
  FILE *f = fopen("/sys/fs/cgroup/cpu.max", "r");
  if (f) {
    char quota[32]; long period = 0;
    if (fscanf(f, "%31s %ld", quota, &period) == 2 && strcmp(quota, "max") != 0 && period > 0) {
      long q = atol(quota) / period;
      if (q < 1) q = 1;
      if (q < n) n = q;
    }
    fclose(f);
  }
  return (int)n;
}
#ifdef _OPENMP
__attribute__((constructor)) static void cap_openmp_team(void) {
  if (getenv("OMP_NUM_THREADS")) return;
  int n = hpgmg_usable_cpus();
  if (n < omp_get_max_threads()) omp_set_num_threads(n);
}
#endif

extern int hpgmg_box_align_jstride, hpgmg_box_align_kstride, hpgmg_box_align_volume, hpgmg_box_align_base_bytes;

static double now(void) {
  struct timespec ts;
  clock_gettime(CLOCK_MONOTONIC, &ts);
  return (double)ts.tv_sec + 1e-9 * (double)ts.tv_nsec;
}
#define SAY(rank, ...) do { if ((rank) == 0 && hpgmg_verbose) { fprintf(stdout, __VA_ARGS__); fflush(stdout); } } while (0)

void hpgmg_set_verbose(int v) { hpgmg_verbose = v; }
void hpgmg_set_box_alignment(int jstride, int kstride, int volume, int base_bytes) {
  if (jstride > 0) hpgmg_box_align_jstride = jstride;
  if (kstride > 0) hpgmg_box_align_kstride = kstride;
  if (volume > 0) hpgmg_box_align_volume = volume;
  if (base_bytes >= 8) hpgmg_box_align_base_bytes = base_bytes;
}

int hpgmg_choose_boxes_in_i(int log2_box_dim, int target_boxes_per_rank, int num_ranks) {
  const long long box_dim = 1LL << log2_box_dim, target = (long long)target_boxes_per_rank * (long long)num_ranks;
  long long bi, best = -1;
  for (bi = 1; bi < 1000; bi++) {
    if (bi * bi * bi > target) continue;
    long long odd = box_dim * bi;
    while ((odd & 1) == 0) odd >>= 1;
    if (odd <= 11) best = bi; /* MAX_COARSE_DIM: the bottom solver must stay small */
  }
  return (int)best;
}

hpgmg_solver *hpgmg_solver_create_explicit(int boxes_in_i, int box_dim, int bc, int my_rank, int num_ranks) {
  hpgmg_config cfg;
  hpgmg_get_config(&cfg);
  hpgmg_solver *s = (hpgmg_solver *)calloc(1, sizeof(*s));
  s->boxes_in_i = boxes_in_i; s->box_dim = box_dim; s->my_rank = my_rank; s->num_ranks = num_ranks;
  create_level(&s->level_h, boxes_in_i, box_dim, stencil_get_radius(), hpgmg_vectors_reserved(), bc, my_rank, num_ranks);
  if (cfg.helmholtz) { s->a = 1.0; s->b = 1.0; SAY(my_rank, "  Creating Helmholtz (a=%f, b=%f) test problem\n", s->a, s->b); }
  else               { s->a = 0.0; s->b = 1.0; SAY(my_rank, "  Creating Poisson (a=%f, b=%f) test problem\n", s->a, s->b); }
  s->h = 1.0 / ((double)boxes_in_i * (double)box_dim);
  initialize_problem(&s->level_h, s->h, s->a, s->b);
  rebuild_operator(&s->level_h, NULL, s->a, s->b);
  if (bc == BC_PERIODIC) {
    double avg = mean(&s->level_h, VECTOR_F);
    if (avg != 0.0) {
      if (my_rank == 0) fprintf(stderr, "  WARNING... Periodic boundary conditions, but f does not sum to zero... mean(f)=%e\n", avg);
      shift_vector(&s->level_h, VECTOR_F, VECTOR_F, -avg);
    }
  }
  MGBuild(&s->mg, &s->level_h, s->a, s->b, bc == BC_PERIODIC ? 2 : 1);
  return s;
}

hpgmg_solver *hpgmg_solver_create(int log2_box_dim, int target_boxes_per_rank, int bc, int my_rank, int num_ranks) {
  int bi = hpgmg_choose_boxes_in_i(log2_box_dim, target_boxes_per_rank, num_ranks);
  if (bi < 1) { if (my_rank == 0) fprintf(stderr, "failed to find an acceptable problem size\n"); return NULL; }
  return hpgmg_solver_create_explicit(bi, 1 << log2_box_dim, bc, my_rank, num_ranks);
}

void hpgmg_solver_destroy(hpgmg_solver *s) {
  if (!s) return;
  MGDestroy(&s->mg);
  destroy_level(&s->level_h);
  free(s);
}

int hpgmg_solver_num_levels(const hpgmg_solver *s) { return s->mg.num_levels; }
mg_type *hpgmg_solver_mg(hpgmg_solver *s) { return &s->mg; }
void hpgmg_solver_coefficients(const hpgmg_solver *s, double ab[2]) { ab[0] = s->a; ab[1] = s->b; }
level_type *hpgmg_solver_level(hpgmg_solver *s, int l) { return (l >= 0 && l < s->mg.num_levels) ? s->mg.levels[l] : NULL; }

void hpgmg_solver_restrict_rhs(hpgmg_solver *s, int l) {
  if (l > 0) restriction(s->mg.levels[l], VECTOR_F, s->mg.levels[l - 1], VECTOR_F, RESTRICT_CELL);
}

static int solve_with_vcycles = 0;      /* --vcycles: the benchmark solves with MGSolve (V-cycles until converged), as the reference built without -DUSE_FCYCLES does (hpgmg-fv.c:79-83) */
double hpgmg_solver_fmg(hpgmg_solver *s, int l) {
  if (solve_with_vcycles) { zero_vector(s->mg.levels[l], VECTOR_U); MGSolve(&s->mg, l, VECTOR_U, VECTOR_F, s->a, s->b, 1e-10); }
  else { hpgmg_fmg_zero_u_first(); FMGSolve(&s->mg, l, VECTOR_U, VECTOR_F, s->a, s->b, 1e-10); }      /* zero_vector(u) + FMGSolve: u is zeroed where FMGSolve first touches it */
  return hpgmg_last_solve.norm_of_residual;
}

double hpgmg_solver_bench(hpgmg_solver *s, int l, int warmup, int solves) {
  int n;
  for (n = 0; n < warmup; n++) hpgmg_solver_fmg(s, l);
  MGResetTimers(&s->mg);
  for (n = 0; n < solves; n++) hpgmg_solver_fmg(s, l);
  return s->mg.timers.MGSolve / (double)(s->mg.MGSolves_performed ? s->mg.MGSolves_performed : 1);
}

void hpgmg_solver_richardson(hpgmg_solver *s, double out[2]) {
  int l;
  MGResetTimers(&s->mg);
  for (l = 0; l < 3; l++) {
    hpgmg_solver_restrict_rhs(s, l);
    hpgmg_solver_fmg(s, l);
  }
  richardson_error(&s->mg, 0, VECTOR_U);
  out[0] = hpgmg_last_solve.richardson_error;
  out[1] = hpgmg_last_solve.richardson_order;
}

/* ------------------------------------------------------------------ dense arrays <-> boxes: host defaults
 * (include/hpgmg_operators.h).  Box by box through the plugin's upload / download; weak, so that a plugin with kernels for it (the HIP plugin:
 * host/plugin_dense.c) replaces them while one without (the CPU oracle, whose memory is host memory for either `where`) gets these. */
static int dense_extent(const level_type *L, int layout, int axis) {
  const int n = axis == 0 ? L->dim.i : axis == 1 ? L->dim.j : L->dim.k;
  return n + (layout == HPGMG_DENSE_FACE_I + axis && L->boundary_condition.type == BC_DIRICHLET);
}
/* mask, wall: hpgmg_dense_pack_walls (0, NULL: hpgmg_dense_pack) */
static int dense_pack_host(level_type *L, int id, const double *src, int where, int layout, int check, int mask, double *wall) {
  if (L->num_ranks != 1 || id < 0 || id >= L->numVectors || layout < HPGMG_DENSE_CELL || layout > HPGMG_DENSE_FACE_K || !src) return -1;
  if (where != HPGMG_WHERE_HOST && where != HPGMG_WHERE_PLUGIN) return -1;
  const int axis = layout - HPGMG_DENSE_FACE_I, n = L->dim.i;
  const int lo = mask ? (mask >> (2 * axis)) & 1 : 0, hi = mask ? (mask >> (2 * axis + 1)) & 1 : 0;
  double *wh = NULL;
  if (lo || hi) { wh = (double *)malloc((size_t)6 * n * n * sizeof(double)); hpgmg_vector_download(wh, wall, (size_t)6 * n * n); }
  const size_t ni = (size_t)dense_extent(L, layout, 0), nj = (size_t)dense_extent(L, layout, 1);
  const int g = L->box_ghosts, dim = L->box_dim, jS = L->box_jStride, kS = L->box_kStride;
  double *box = (double *)malloc((size_t)L->box_volume * sizeof(double));
  int b, i, j, k, status = 0;
  for (b = 0; b < L->num_my_boxes; b++) {
    const box_type *B = &L->my_boxes[b];
    /* the high ghost layer along the array's axis belongs to it on the domain's high face (Dirichlet face arrays) */
    const int ei = dim + (ni > (size_t)L->dim.i && B->low.i + dim == L->dim.i);
    const int ej = dim + (nj > (size_t)L->dim.j && B->low.j + dim == L->dim.j);
    const int ek = dim + (dense_extent(L, layout, 2) > L->dim.k && B->low.k + dim == L->dim.k);
    memset(box, 0, (size_t)L->box_volume * sizeof(double));
    for (k = 0; k < ek; k++) for (j = 0; j < ej; j++) for (i = 0; i < ei; i++) {
      const double v = src[((size_t)(B->low.k + k) * nj + (size_t)(B->low.j + j)) * ni + (size_t)(B->low.i + i)];
      if (!isfinite(v)) status |= HPGMG_DENSE_NOT_FINITE;
      else if ((check == HPGMG_DENSE_CHECK_POSITIVE && !(v > 0.0)) || (check == HPGMG_DENSE_CHECK_NONNEGATIVE && !(v >= 0.0))) status |= HPGMG_DENSE_OUT_OF_RANGE;
      const int c = axis == 0 ? i : axis == 1 ? j : k, gc = (axis == 0 ? B->low.i : axis == 1 ? B->low.j : B->low.k) + c;
      if ((lo && gc == 0) || (hi && gc == n)) {               /* a masked domain wall: its beta goes to the wall array, the vector takes 0.0 */
        const int q = axis == 2 ? B->low.j + j : B->low.k + k, p = axis == 0 ? B->low.j + j : B->low.i + i;
        wh[((size_t)(2 * axis + (gc == n)) * n + q) * n + p] = v;
        box[(i + g) + (j + g) * jS + (k + g) * kS] = 0.0;
      } else
      box[(i + g) + (j + g) * jS + (k + g) * kS] = v;
    }
    hpgmg_vector_upload(B->vectors[id], box, (size_t)L->box_volume);
  }
  free(box);
  if (wh) { hpgmg_vector_upload(wall, wh, (size_t)6 * n * n); free(wh); }
  return status;
}
__attribute__((weak)) int hpgmg_dense_pack(level_type *L, int id, const double *src, int where, int layout, int check) {
  return dense_pack_host(L, id, src, where, layout, check, 0, NULL);
}
__attribute__((weak)) int hpgmg_dense_pack_walls(level_type *L, int id, const double *src, int where, int layout, int check, int mask, double *wall) {
  if (layout < HPGMG_DENSE_FACE_I || !wall || mask < 0 || mask > 63 || L->boundary_condition.type != BC_DIRICHLET || L->dim.i != L->dim.j || L->dim.i != L->dim.k) return -1;
  return dense_pack_host(L, id, src, where, layout, check, mask, wall);
}
__attribute__((weak)) int hpgmg_dense_unpack(level_type *L, int id, double *dst, int where) {
  if (L->num_ranks != 1 || id < 0 || id >= L->numVectors || !dst) return -1;
  if (where != HPGMG_WHERE_HOST && where != HPGMG_WHERE_PLUGIN) return -1;
  const size_t ni = (size_t)L->dim.i, nj = (size_t)L->dim.j;
  const int g = L->box_ghosts, dim = L->box_dim, jS = L->box_jStride, kS = L->box_kStride;
  double *box = (double *)malloc((size_t)L->box_volume * sizeof(double));
  int b, i, j, k;
  for (b = 0; b < L->num_my_boxes; b++) {
    const box_type *B = &L->my_boxes[b];
    hpgmg_vector_download(box, B->vectors[id], (size_t)L->box_volume);
    for (k = 0; k < dim; k++) for (j = 0; j < dim; j++) for (i = 0; i < dim; i++)
      dst[((size_t)(B->low.k + k) * nj + (size_t)(B->low.j + j)) * ni + (size_t)(B->low.i + i)] = box[(i + g) + (j + g) * jS + (k + g) * kS];
  }
  free(box);
  return 0;
}

/* ------------------------------------------------------------------ boundary values: host defaults (include/hpgmg_operators.h)
 * Box by box through hpgmg_vector_upload / download, weak like the dense pair above (the HIP plugin: host/plugin_dense.c).  The domain is the
 * user problems' cube of n = dim.i cells per side. */
static int bnd_touches(int n, int face, int gi, int gj, int gk) {          /* cell (gi,gj,gk) lies on domain face `face` */
  const int c = face < 2 ? gi : face < 4 ? gj : gk;
  return (face & 1) ? c == n - 1 : c == 0;
}
static size_t bnd_entry(int n, int face, int gi, int gj, int gk) {         /* its entry in a 6 x n x n boundary array */
  const int q = face < 4 ? gk : gj, p = face < 2 ? gj : gi;
  return ((size_t)face * n + q) * n + p;
}
static int bnd_box_on_domain_face(const level_type *L, const box_type *B) {
  const int n = L->dim.i, d = L->box_dim;
  return B->low.i == 0 || B->low.j == 0 || B->low.k == 0 || B->low.i + d == n || B->low.j + d == n || B->low.k + d == n;
}
/* beta of domain face `face` of the box cell at padded offset ijk */
static double bnd_beta(const double *bi, const double *bj, const double *bk, int face, int ijk, int jS, int kS) {
  switch (face) {
    case 0: return bi[ijk];  case 1: return bi[ijk + 1];
    case 2: return bj[ijk];  case 3: return bj[ijk + jS];
    case 4: return bk[ijk];  default: return bk[ijk + kS];
  }
}
static double bnd_weight(const level_type *L, double b) { return (2.0 * b) * (1.0 / (L->h * L->h)); }
/* S(c) of hpgmg_boundary_lift: the four finer entries under each face entry of coarse cell (gi,gj,gk), faces in order */
static double bnd_fine_sum(int n, const double *phi_f, int gi, int gj, int gk) {
  double S = 0.0;
  int face;
  for (face = 0; face < 6; face++) if (bnd_touches(n, face, gi, gj, gk)) {
    const int q = face < 4 ? gk : gj, p = face < 2 ? gj : gi;
    const double *e = phi_f + ((size_t)face * 2 * n + 2 * q) * 2 * n + 2 * p;
    S = S + (((e[0] + e[1]) + e[2 * n]) + e[2 * n + 1]);
  }
  return S;
}
static double *bnd_download(const double *src, size_t n) {
  double *h = (double *)malloc(n * sizeof(double));
  hpgmg_vector_download(h, src, n);
  return h;
}

static double bnd_weight_neumann(const level_type *L, double b) { return b * (1.0 / L->h); }
/* mask, wall: hpgmg_dense_pack_lifted_faces (0, NULL: hpgmg_dense_pack_lifted) */
static int dense_pack_lifted_host(level_type *L, int id, const double *f, int where, const double *g, double b, int mask, const double *wall) {
  if (!g || L->boundary_condition.type != BC_DIRICHLET) return -1;
  const int st = hpgmg_dense_pack(L, id, f, where, HPGMG_DENSE_CELL, HPGMG_DENSE_CHECK_FINITE);
  if (st < 0) return st;
  const int n = L->dim.i, g0 = L->box_ghosts, dim = L->box_dim, jS = L->box_jStride, kS = L->box_kStride;
  const double w = bnd_weight(L, b), wn = bnd_weight_neumann(L, b);
  double *gh = bnd_download(g, (size_t)6 * n * n), *wh = mask ? bnd_download(wall, (size_t)6 * n * n) : NULL;
  double *v = (double *)malloc((size_t)L->box_volume * 4 * sizeof(double));
  double *bi = v + L->box_volume, *bj = bi + L->box_volume, *bk = bj + L->box_volume;
  int box, i, j, k, face, bad = 0;
  for (box = 0; box < L->num_my_boxes; box++) {
    const box_type *B = &L->my_boxes[box];
    if (!bnd_box_on_domain_face(L, B)) continue;
    hpgmg_vector_download(v, B->vectors[id], (size_t)L->box_volume);
    hpgmg_vector_download(bi, B->vectors[VECTOR_BETA_I], (size_t)L->box_volume);
    hpgmg_vector_download(bj, B->vectors[VECTOR_BETA_J], (size_t)L->box_volume);
    hpgmg_vector_download(bk, B->vectors[VECTOR_BETA_K], (size_t)L->box_volume);
    for (k = 0; k < dim; k++) for (j = 0; j < dim; j++) for (i = 0; i < dim; i++) {
      const int gi = B->low.i + i, gj = B->low.j + j, gk = B->low.k + k, ijk = (i + g0) + (j + g0) * jS + (k + g0) * kS;
      double T = 0.0;
      int on = 0;
      for (face = 0; face < 6; face++) if (bnd_touches(n, face, gi, gj, gk)) {
        const double gv = gh[bnd_entry(n, face, gi, gj, gk)];
        if (!isfinite(gv)) bad = 1;
        if ((mask >> face) & 1) T = T + (wn * wh[bnd_entry(n, face, gi, gj, gk)]) * gv;
        else T = T + (w * bnd_beta(bi, bj, bk, face, ijk, jS, kS)) * gv;
        on = 1;
      }
      if (on) v[ijk] = v[ijk] + T;
    }
    hpgmg_vector_upload(B->vectors[id], v, (size_t)L->box_volume);
  }
  free(v); free(gh); free(wh);
  return st | (bad ? HPGMG_DENSE_NOT_FINITE : 0);
}
__attribute__((weak)) int hpgmg_dense_pack_lifted(level_type *L, int id, const double *f, int where, const double *g, double b) {
  return dense_pack_lifted_host(L, id, f, where, g, b, 0, NULL);
}
__attribute__((weak)) int hpgmg_dense_pack_lifted_faces(level_type *L, int id, const double *f, int where, const double *g, double b, int mask, const double *wall) {
  if (mask < 0 || mask > 63 || (mask && !wall)) return -1;
  return dense_pack_lifted_host(L, id, f, where, g, b, mask, wall);
}

static int boundary_flux_host(level_type *L, double *phi, const double *g, double b, int mask, const double *wall) {
  const int n = L->dim.i, g0 = L->box_ghosts, dim = L->box_dim, jS = L->box_jStride, kS = L->box_kStride;
  const size_t len = (size_t)6 * n * n;
  const double w = bnd_weight(L, b), wn = bnd_weight_neumann(L, b);
  double *gh = bnd_download(g, len), *ph = (double *)calloc(len, sizeof(double)), *wh = mask ? bnd_download(wall, len) : NULL;
  double *bi = (double *)malloc((size_t)L->box_volume * 3 * sizeof(double)), *bj = bi + L->box_volume, *bk = bj + L->box_volume;
  int box, i, j, k, face, bad = 0;
  size_t e;
  for (e = 0; e < len; e++) if (!isfinite(gh[e])) bad = 1;
  for (box = 0; box < L->num_my_boxes; box++) {
    const box_type *B = &L->my_boxes[box];
    if (!bnd_box_on_domain_face(L, B)) continue;
    hpgmg_vector_download(bi, B->vectors[VECTOR_BETA_I], (size_t)L->box_volume);
    hpgmg_vector_download(bj, B->vectors[VECTOR_BETA_J], (size_t)L->box_volume);
    hpgmg_vector_download(bk, B->vectors[VECTOR_BETA_K], (size_t)L->box_volume);
    for (k = 0; k < dim; k++) for (j = 0; j < dim; j++) for (i = 0; i < dim; i++) {
      const int gi = B->low.i + i, gj = B->low.j + j, gk = B->low.k + k, ijk = (i + g0) + (j + g0) * jS + (k + g0) * kS;
      for (face = 0; face < 6; face++) if (bnd_touches(n, face, gi, gj, gk)) {
        e = bnd_entry(n, face, gi, gj, gk);
        if ((mask >> face) & 1) ph[e] = (wn * wh[e]) * gh[e];
        else ph[e] = (w * bnd_beta(bi, bj, bk, face, ijk, jS, kS)) * gh[e];
      }
    }
  }
  hpgmg_vector_upload(phi, ph, len);
  free(bi); free(ph); free(gh); free(wh);
  return bad ? HPGMG_DENSE_NOT_FINITE : 0;
}
__attribute__((weak)) int hpgmg_boundary_flux(level_type *L, double *phi, const double *g, double b) { return boundary_flux_host(L, phi, g, b, 0, NULL); }
__attribute__((weak)) int hpgmg_boundary_flux_faces(level_type *L, double *phi, const double *g, double b, int mask, const double *wall) {
  if (mask < 0 || mask > 63 || (mask && !wall)) return -1;
  return boundary_flux_host(L, phi, g, b, mask, wall);
}

__attribute__((weak)) void hpgmg_boundary_restrict(level_type *Lc, double *g_c, level_type *Lf, const double *g_f) {
  const int nc = Lc->dim.i, nf = Lf->dim.i;
  double *gf = bnd_download(g_f, (size_t)6 * nf * nf), *gc = (double *)malloc((size_t)6 * nc * nc * sizeof(double));
  int face, q, p;
  for (face = 0; face < 6; face++) for (q = 0; q < nc; q++) for (p = 0; p < nc; p++) {
    const double *e = gf + ((size_t)face * nf + 2 * q) * nf + 2 * p;
    gc[((size_t)face * nc + q) * nc + p] = (e[0] + e[1] + e[nf] + e[nf + 1]) * 0.25;
  }
  hpgmg_vector_upload(g_c, gc, (size_t)6 * nc * nc);
  free(gc); free(gf);
}

__attribute__((weak)) void hpgmg_boundary_lift(level_type *L, int id, const double *phi, const double *phi_fine, double sign) {
  const int n = L->dim.i, g0 = L->box_ghosts, dim = L->box_dim, jS = L->box_jStride, kS = L->box_kStride;
  double *ph = bnd_download(phi, (size_t)6 * n * n), *pf = phi_fine ? bnd_download(phi_fine, (size_t)24 * n * n) : NULL;
  double *v = (double *)malloc((size_t)L->box_volume * sizeof(double));
  int box, i, j, k, face;
  for (box = 0; box < L->num_my_boxes; box++) {
    const box_type *B = &L->my_boxes[box];
    if (!bnd_box_on_domain_face(L, B)) continue;
    hpgmg_vector_download(v, B->vectors[id], (size_t)L->box_volume);
    for (k = 0; k < dim; k++) for (j = 0; j < dim; j++) for (i = 0; i < dim; i++) {
      const int gi = B->low.i + i, gj = B->low.j + j, gk = B->low.k + k, ijk = (i + g0) + (j + g0) * jS + (k + g0) * kS;
      double T = 0.0;
      int on = 0;
      for (face = 0; face < 6; face++) if (bnd_touches(n, face, gi, gj, gk)) { T = T + ph[bnd_entry(n, face, gi, gj, gk)]; on = 1; }
      if (!on) continue;
      if (pf) T = T - 0.125 * bnd_fine_sum(n, pf, gi, gj, gk);
      v[ijk] = v[ijk] + sign * T;
    }
    hpgmg_vector_upload(B->vectors[id], v, (size_t)L->box_volume);
  }
  free(v); free(pf); free(ph);
}

/* delta of the ghost at coarse (ci,cj,ck) (hpgmg_boundary_interp): 2 g on a face, the wall-by-wall linear rule on an edge
 * or corner (exact for u linear near them).  BND_AT(face, i, j, k): the entry of `face` at the in-range cell (i, j, k) (its own axis not read). */
#define BND_AT(f, i, j, k) g[((size_t)(f) * n + ((f) < 4 ? (k) : (j))) * n + ((f) < 2 ? (j) : (i))]
static double bnd_ghost_delta(int n, const double *g, int ci, int cj, int ck) {
  const int q[3] = { ci, cj, ck };
  int out[3], P[3], step[3], face[3], a, m = 0;
  for (a = 0; a < 3; a++) {
    out[a] = q[a] < 0 || q[a] >= n;
    P[a] = q[a] < 0 ? 0 : q[a] >= n ? n - 1 : q[a];
    step[a] = q[a] < 0 ? 1 : -1;                               /* one cell inward */
    face[a] = 2 * a + (q[a] >= n);
    m += out[a];
  }
  if (m == 1) { a = out[0] ? 0 : out[1] ? 1 : 2; return 2.0 * BND_AT(face[a], P[0], P[1], P[2]); }
  if (n < 2) return m == 3 ? ((BND_AT(face[0], P[0], P[1], P[2]) + BND_AT(face[1], P[0], P[1], P[2])) + BND_AT(face[2], P[0], P[1], P[2])) * (2.0 / 3.0) : 0.0;
  if (m == 2) {                      /* the outside axes x < y: each wall's entry next to the edge minus the one a cell further along the other wall */
    const int x = out[0] ? 0 : 1, y = out[2] ? 2 : 1;
    const int yi = P[0] + (y == 0) * step[0], yj = P[1] + (y == 1) * step[1], yk = P[2] + (y == 2) * step[2];
    const int xi = P[0] + (x == 0) * step[0], xj = P[1] + (x == 1) * step[1], xk = P[2] + (x == 2) * step[2];
    return (BND_AT(face[x], P[0], P[1], P[2]) - BND_AT(face[x], yi, yj, yk)) + (BND_AT(face[y], P[0], P[1], P[2]) - BND_AT(face[y], xi, xj, xk));
  }
  double c[3];                       /* corner: each wall's linear extrapolation to the corner point */
  for (a = 0; a < 3; a++) {
    const int b = a == 0 ? 1 : 0, d = a == 2 ? 1 : 2;          /* the wall's in-face axes, b < d */
    const double g00 = BND_AT(face[a], P[0], P[1], P[2]);
    const double g10 = BND_AT(face[a], P[0] + (b == 0) * step[0], P[1] + (b == 1) * step[1], P[2]);
    const double g01 = BND_AT(face[a], P[0], P[1] + (d == 1) * step[1], P[2] + (d == 2) * step[2]);
    c[a] = (2.0 * g00 - 0.5 * g10) - 0.5 * g01;
  }
  return ((c[0] + c[1]) + c[2]) * (2.0 / 3.0);
}
#undef BND_AT
/* D(c) of hpgmg_boundary_interp for fine cell (gi,gj,gk): the p1 weights of its ghost reads times their deltas, in interpolation_p1's order */
static double bnd_interp_delta(int nc, const double *g, int gi, int gj, int gk) {
  const int ci = gi >> 1, cj = gj >> 1, ck = gk >> 1, di = (gi & 1) ? 1 : -1, dj = (gj & 1) ? 1 : -1, dk = (gk & 1) ? 1 : -1;
  static const double w[8] = { 0.421875, 0.140625, 0.140625, 0.046875, 0.140625, 0.046875, 0.046875, 0.015625 };
  static const int si[8] = { 0, 0, 0, 0, 1, 1, 1, 1 }, sj[8] = { 0, 0, 1, 1, 0, 0, 1, 1 }, sk[8] = { 0, 1, 0, 1, 0, 1, 0, 1 };
  double D = 0.0;
  int t;
  for (t = 1; t < 8; t++) {
    const int qi = ci + si[t] * di, qj = cj + sj[t] * dj, qk = ck + sk[t] * dk;
    if (qi < 0 || qi >= nc || qj < 0 || qj >= nc || qk < 0 || qk >= nc) D = D + w[t] * bnd_ghost_delta(nc, g, qi, qj, qk);
  }
  return D;
}

/* hpgmg_boundary_interp_faces' delta (include/hpgmg_operators.h): u the coarse iterate as a dense (n,n,n) array, hc the coarse h */
#define BND_AT(f, i, j, k) g[((size_t)(f) * n + ((f) < 4 ? (k) : (j))) * n + ((f) < 2 ? (j) : (i))]
static double bnd_ghost_delta_faces(int n, const double *g, const double *u, double hc, int mask, int ci, int cj, int ck) {
  const int q[3] = { ci, cj, ck };
  int out[3], P[3], face[3], a, m = 0, dirichlet = 0;
  for (a = 0; a < 3; a++) {
    out[a] = q[a] < 0 || q[a] >= n;
    P[a] = q[a] < 0 ? 0 : q[a] >= n ? n - 1 : q[a];
    face[a] = 2 * a + (q[a] >= n);
    m += out[a];
    dirichlet += out[a] && !((mask >> face[a]) & 1);
  }
  if (dirichlet == m) return bnd_ghost_delta(n, g, ci, cj, ck);
  double s = 0.0;
  for (a = 0; a < 3; a++) if (out[a]) {
    const double ga = BND_AT(face[a], P[0], P[1], P[2]);
    s = s + (((mask >> face[a]) & 1) ? hc * ga : 2.0 * ga);
  }
  const double c = (double)(1 - 2 * dirichlet + ((m & 1) ? 1 : -1));
  return c * u[((size_t)P[2] * n + P[1]) * n + P[0]] + s;
}
#undef BND_AT
static double bnd_interp_delta_faces(int nc, const double *g, const double *u, double hc, int mask, int gi, int gj, int gk) {
  const int ci = gi >> 1, cj = gj >> 1, ck = gk >> 1, di = (gi & 1) ? 1 : -1, dj = (gj & 1) ? 1 : -1, dk = (gk & 1) ? 1 : -1;
  static const double w[8] = { 0.421875, 0.140625, 0.140625, 0.046875, 0.140625, 0.046875, 0.046875, 0.015625 };
  static const int si[8] = { 0, 0, 0, 0, 1, 1, 1, 1 }, sj[8] = { 0, 0, 1, 1, 0, 0, 1, 1 }, sk[8] = { 0, 1, 0, 1, 0, 1, 0, 1 };
  double D = 0.0;
  int t;
  for (t = 1; t < 8; t++) {
    const int qi = ci + si[t] * di, qj = cj + sj[t] * dj, qk = ck + sk[t] * dk;
    if (qi < 0 || qi >= nc || qj < 0 || qj >= nc || qk < 0 || qk >= nc) D = D + w[t] * bnd_ghost_delta_faces(nc, g, u, hc, mask, qi, qj, qk);
  }
  return D;
}

__attribute__((weak)) void hpgmg_boundary_interp_faces(level_type *Lf, int id, level_type *Lc, const double *g_c, int mask) {
  const int n = Lf->dim.i, nc = Lc->dim.i, g0 = Lf->box_ghosts, dim = Lf->box_dim, jS = Lf->box_jStride, kS = Lf->box_kStride;
  double *gc = bnd_download(g_c, (size_t)6 * nc * nc), *v = (double *)malloc((size_t)Lf->box_volume * sizeof(double));
  double *uc = (double *)malloc((size_t)nc * nc * nc * sizeof(double));
  int box, i, j, k;
  hpgmg_dense_unpack(Lc, id, uc, HPGMG_WHERE_HOST);
  for (box = 0; box < Lf->num_my_boxes; box++) {
    const box_type *B = &Lf->my_boxes[box];
    if (!bnd_box_on_domain_face(Lf, B)) continue;
    hpgmg_vector_download(v, B->vectors[id], (size_t)Lf->box_volume);
    for (k = 0; k < dim; k++) for (j = 0; j < dim; j++) for (i = 0; i < dim; i++) {
      const int gi = B->low.i + i, gj = B->low.j + j, gk = B->low.k + k, ijk = (i + g0) + (j + g0) * jS + (k + g0) * kS;
      if (gi > 0 && gj > 0 && gk > 0 && gi < n - 1 && gj < n - 1 && gk < n - 1) continue;
      v[ijk] = v[ijk] + bnd_interp_delta_faces(nc, gc, uc, Lc->h, mask, gi, gj, gk);
    }
    hpgmg_vector_upload(B->vectors[id], v, (size_t)Lf->box_volume);
  }
  free(uc); free(v); free(gc);
}

__attribute__((weak)) void hpgmg_boundary_interp(level_type *Lf, int id, level_type *Lc, const double *g_c) {
  const int n = Lf->dim.i, nc = Lc->dim.i, g0 = Lf->box_ghosts, dim = Lf->box_dim, jS = Lf->box_jStride, kS = Lf->box_kStride;
  double *gc = bnd_download(g_c, (size_t)6 * nc * nc), *v = (double *)malloc((size_t)Lf->box_volume * sizeof(double));
  int box, i, j, k;
  for (box = 0; box < Lf->num_my_boxes; box++) {
    const box_type *B = &Lf->my_boxes[box];
    if (!bnd_box_on_domain_face(Lf, B)) continue;
    hpgmg_vector_download(v, B->vectors[id], (size_t)Lf->box_volume);
    for (k = 0; k < dim; k++) for (j = 0; j < dim; j++) for (i = 0; i < dim; i++) {
      const int gi = B->low.i + i, gj = B->low.j + j, gk = B->low.k + k, ijk = (i + g0) + (j + g0) * jS + (k + g0) * kS;
      if (gi > 0 && gj > 0 && gk > 0 && gi < n - 1 && gj < n - 1 && gk < n - 1) continue;
      v[ijk] = v[ijk] + bnd_interp_delta(nc, gc, gi, gj, gk);
    }
    hpgmg_vector_upload(B->vectors[id], v, (size_t)Lf->box_volume);
  }
  free(v); free(gc);
}

/* ------------------------------------------------------------------ the CG passes: portable forms (include/hpgmg_operators.h)
 * The operators, then the sums on the host from downloaded boxes, in the one order the header defines.  The hooks are weak like the dense pair above:
 * the HIP plugin (host/plugin_pcg.c) replaces them with its kernels and comes back to the _host forms on a level those do not take. */
typedef struct { double *V; size_t W, S, len; } pcg_leaves;
static pcg_leaves pcg_leaves_of(const level_type *L) {
  pcg_leaves P;
  const size_t dim = (size_t)L->box_dim, used = HPGMG_PCG_COLUMNS * ((dim * dim + HPGMG_PCG_COLUMNS - 1) / HPGMG_PCG_COLUMNS);
  P.W = used; P.S = (dim + HPGMG_PCG_SEGMENT - 1) / HPGMG_PCG_SEGMENT;
  for (P.len = 1; P.len < P.W * P.S * (size_t)L->num_my_boxes; P.len *= 2) {}
  P.V = (double *)calloc(P.len, sizeof(double));
  return P;
}
static double pcg_fold(pcg_leaves *P) {
  size_t stride, m;
  for (stride = 1; stride < P->len; stride *= 2)
    for (m = 0; m + stride < P->len; m += 2 * stride) P->V[m] = P->V[m] + P->V[m + stride];
  const double sum = P->V[0];
  free(P->V);
  return sum;
}
/* the leaves of box bx: per column and segment the chain over its planes of the products va * vb */
static void pcg_box_leaves(const level_type *L, pcg_leaves *P, int bx, const double *va, const double *vb) {
  const int g = L->box_ghosts, dim = L->box_dim, jS = L->box_jStride, kS = L->box_kStride;
  int i, j, k;
  size_t s;
  for (s = 0; s < P->S; s++) for (j = 0; j < dim; j++) for (i = 0; i < dim; i++) {
    const int k1 = (int)(s + 1) * HPGMG_PCG_SEGMENT < dim ? (int)(s + 1) * HPGMG_PCG_SEGMENT : dim;
    double chain = 0.0;
    for (k = (int)s * HPGMG_PCG_SEGMENT; k < k1; k++) {
      const int ijk = (i + g) + (j + g) * jS + (k + g) * kS;
      const double q = va[ijk] * vb[ijk];
      chain = chain + q;
    }
    P->V[(size_t)(i + dim * j) + P->W * (s + P->S * (size_t)bx)] = chain;
  }
}
int hpgmg_pcg_dot_host(level_type *L, int a_id, int b_id, double *dot) {
  double *va = (double *)malloc((size_t)L->box_volume * sizeof(double)), *vb = (double *)malloc((size_t)L->box_volume * sizeof(double));
  pcg_leaves P = pcg_leaves_of(L);
  int bx;
  for (bx = 0; bx < L->num_my_boxes; bx++) {
    hpgmg_vector_download(va, L->my_boxes[bx].vectors[a_id], (size_t)L->box_volume);
    hpgmg_vector_download(vb, L->my_boxes[bx].vectors[b_id], (size_t)L->box_volume);
    pcg_box_leaves(L, &P, bx, va, vb);
  }
  free(va); free(vb);
  *dot = pcg_fold(&P);
  return 0;
}
/* a . b and c . b from one download of b: two trees of the one order, so each has the bits of hpgmg_pcg_dot_host on its pair */
int hpgmg_pcg_dot2_host(level_type *L, int a_id, int c_id, int b_id, double *ab, double *cb) {
  const size_t vol = (size_t)L->box_volume;
  double *v = (double *)malloc(3 * vol * sizeof(double)), *va = v, *vc = v + vol, *vb = v + 2 * vol;
  pcg_leaves P = pcg_leaves_of(L), Q = pcg_leaves_of(L);
  int bx;
  for (bx = 0; bx < L->num_my_boxes; bx++) {
    hpgmg_vector_download(va, L->my_boxes[bx].vectors[a_id], vol);
    hpgmg_vector_download(vc, L->my_boxes[bx].vectors[c_id], vol);
    hpgmg_vector_download(vb, L->my_boxes[bx].vectors[b_id], vol);
    pcg_box_leaves(L, &P, bx, va, vb);
    pcg_box_leaves(L, &Q, bx, vc, vb);
  }
  free(v);
  *ab = pcg_fold(&P);
  *cb = pcg_fold(&Q);
  return 0;
}
int hpgmg_pcg_apply_dot_host(level_type *L, int Ap_id, int p_id, double a, double b, double *dot) {
  apply_op(L, Ap_id, p_id, a, b);
  return hpgmg_pcg_dot_host(L, p_id, Ap_id, dot);
}
int hpgmg_pcg_update_host(level_type *L, int x_id, int r_id, int p_id, int Ap_id, double alpha, double *rmax) {
  const int g = L->box_ghosts, dim = L->box_dim, jS = L->box_jStride, kS = L->box_kStride;
  const size_t vol = (size_t)L->box_volume;
  double *v = (double *)malloc(4 * vol * sizeof(double)), *x = v, *r = v + vol, *p = v + 2 * vol, *Ap = v + 3 * vol;
  double best = 0.0;
  int bx, i, j, k;
  for (bx = 0; bx < L->num_my_boxes; bx++) {
    const box_type *B = &L->my_boxes[bx];
    hpgmg_vector_download(x, B->vectors[x_id], vol); hpgmg_vector_download(r, B->vectors[r_id], vol);
    hpgmg_vector_download(p, B->vectors[p_id], vol); hpgmg_vector_download(Ap, B->vectors[Ap_id], vol);
    for (k = 0; k < dim; k++) for (j = 0; j < dim; j++) for (i = 0; i < dim; i++) {
      const int ijk = (i + g) + (j + g) * jS + (k + g) * kS;
      const double dx = alpha * p[ijk], dr = alpha * Ap[ijk];
      x[ijk] = x[ijk] + dx;
      r[ijk] = r[ijk] - dr;
      const double f = fabs(r[ijk]);
      if (f > best) best = f;
    }
    hpgmg_vector_upload(B->vectors[x_id], x, vol); hpgmg_vector_upload(B->vectors[r_id], r, vol);
  }
  free(v);
  *rmax = best;
  return 0;
}
__attribute__((weak)) int hpgmg_pcg_apply_dot(level_type *L, int Ap_id, int p_id, double a, double b, double *dot) { return hpgmg_pcg_apply_dot_host(L, Ap_id, p_id, a, b, dot); }
__attribute__((weak)) int hpgmg_pcg_update(level_type *L, int x_id, int r_id, int p_id, int Ap_id, double alpha, double *rmax) { return hpgmg_pcg_update_host(L, x_id, r_id, p_id, Ap_id, alpha, rmax); }
__attribute__((weak)) int hpgmg_pcg_dot(level_type *L, int a_id, int b_id, double *dot) { return hpgmg_pcg_dot_host(L, a_id, b_id, dot); }
__attribute__((weak)) int hpgmg_pcg_dot2(level_type *L, int a_id, int c_id, int b_id, double *ab, double *cb) { return hpgmg_pcg_dot2_host(L, a_id, c_id, b_id, ab, cb); }

/* ------------------------------------------------------------------ user problems on dense arrays (include/hpgmg_fv.h) */
struct hpgmg_user_solver {
  hpgmg_solver s;              /* the finest level, the hierarchy, a, b, h */
  int n, bc, verbose;
  int x_id;                    /* the finest level's one extra vector: u0 of a warm start, the operand of apply */
  int operator_ok, rhs_ok;     /* 0 after a set_coefficients / set_rhs that was refused part way */
  double mean_shift;           /* what the last set_rhs subtracted from f */
  int bnd;                     /* 1: f was set with boundary values (set_rhs_dirichlet): an F-cycle runs with the hook below */
  double **bnd_g, **bnd_phi;   /* per level: the boundary values g_l and their lift flux phi_l (plugin memory; allocated on first use) */
  double *app_g, *app_phi;     /* apply_dirichlet's g and phi on the finest level */
  int max_iter;                /* HPGMG_USER_PCG / _FPCG: the iteration limit (hpgmg_user_set_max_iterations; default 100) */
  int mask;                    /* bit f: domain face f is a Neumann wall (hpgmg_user_create_faces); 0: every wall Dirichlet, or periodic */
  double *wall0, **wall;       /* mask != 0: wall0 = wall[0]; per level, the wall beta of the Neumann faces (a boundary array; the level's own beta is 0 there) */
};
static int user_live = 0;              /* user solvers alive: the process-wide configuration belongs to them */
static hpgmg_config user_cfg;

/* user calls print only when the solver's verbose flag is on (the library's default, hpgmg_verbose = 1, is the benchmark's) */
#define USER_QUIET(us) const int verbose_saved_ = hpgmg_verbose; hpgmg_verbose = (us)->verbose
#define USER_LOUD() hpgmg_verbose = verbose_saved_

static int user_config_ok(void) {                 /* nobody has reconfigured the process under the live user solvers */
  hpgmg_config cfg;
  hpgmg_get_config(&cfg);
  return cfg.op == user_cfg.op && cfg.smoother == user_cfg.smoother && cfg.helmholtz == user_cfg.helmholtz && cfg.variable_coeff == user_cfg.variable_coeff;
}
static int user_pack_status(int st) {
  if (st < 0) return HPGMG_USER_BAD_ARGUMENT;
  if (st & HPGMG_DENSE_NOT_FINITE) return HPGMG_USER_NOT_FINITE;
  if (st & HPGMG_DENSE_OUT_OF_RANGE) return HPGMG_USER_OUT_OF_RANGE;
  return HPGMG_USER_OK;
}

static void user_bnd_alloc(hpgmg_user_solver *us);
/* a face array of the coefficients into the finest level: with Neumann walls through the masked pack, which keeps their beta in wall[0] */
static int user_pack_beta(hpgmg_user_solver *us, int id, const double *src, int where, int layout) {
  level_type *L = &us->s.level_h;
  if (!us->mask) return hpgmg_dense_pack(L, id, src, where, layout, HPGMG_DENSE_CHECK_POSITIVE);
  return hpgmg_dense_pack_walls(L, id, src, where, layout, HPGMG_DENSE_CHECK_POSITIVE, us->mask, us->wall0);
}
/* after rebuild_operator + MGRebuildCoarse of a solver with Neumann walls: every level's wall beta, and the singular case.  Six Neumann walls
 * without an a * alpha term leave the constants in the null space, as periodic Poisson does: the same path (MGRebuildCoarse has just reset it) */
static void user_walls_rebuilt(hpgmg_user_solver *us) {
  mg_type *G = &us->s.mg;
  int l;
  if (!us->mask) return;
  for (l = 1; l < G->num_levels; l++) hpgmg_boundary_restrict(G->levels[l], us->wall[l], G->levels[l - 1], us->wall[l - 1]);
  if (us->mask != 63) return;
  for (l = 0; l < G->num_levels; l++) {
    level_type *L = G->levels[l];
    int alpha_is_zero = 1;
    if (hpgmg_vectors_reserved() > VECTOR_ALPHA && L->active) alpha_is_zero = (dot(L, VECTOR_ALPHA, VECTOR_ALPHA) == 0.0);
    if (us->s.a == 0 || alpha_is_zero) L->must_subtract_mean = 1;
  }
}

static int user_create(int n, int box_dim, int bc, int mask, int op, int smoother, double a, double b, double h, hpgmg_user_solver **out);
int hpgmg_user_create(int n, int box_dim, int bc, int op, int smoother, double a, double b, double h, hpgmg_user_solver **out) {
  return user_create(n, box_dim, bc, 0, op, smoother, a, b, h, out);
}
int hpgmg_user_create_faces(int n, int box_dim, const int face_bc[6], int op, int smoother, double a, double b, double h, hpgmg_user_solver **out) {
  int f, mask = 0;
  if (out) *out = NULL;
  if (!face_bc) return HPGMG_USER_BAD_ARGUMENT;
  for (f = 0; f < 6; f++) {
    if (face_bc[f] != HPGMG_FACE_DIRICHLET && face_bc[f] != HPGMG_FACE_NEUMANN) return HPGMG_USER_BAD_ARGUMENT;
    if (face_bc[f] == HPGMG_FACE_NEUMANN) mask |= 1 << f;
  }
  return user_create(n, box_dim, BC_DIRICHLET, mask, op, smoother, a, b, h, out);       /* mask 0 is hpgmg_user_create's solver */
}

static int user_create(int n, int box_dim, int bc, int mask, int op, int smoother, double a, double b, double h, hpgmg_user_solver **out) {
  const hpgmg_transport *T = hpgmg_get_transport();
  if (!out) return HPGMG_USER_BAD_ARGUMENT;
  *out = NULL;
  if (op != HPGMG_OP_7PT) return HPGMG_USER_UNSUPPORTED;
  if (T && T->size > 1) return HPGMG_USER_MULTI_RANK;
  if (box_dim <= 0) for (box_dim = 128; box_dim > 1 && n % box_dim; box_dim /= 2) {}
  if (n < 4 || box_dim < 4 || (box_dim & (box_dim - 1)) || box_dim > 512 || n % box_dim) return HPGMG_USER_BAD_ARGUMENT;
  if (bc != BC_DIRICHLET && bc != BC_PERIODIC) return HPGMG_USER_BAD_ARGUMENT;
  if (smoother < HPGMG_SMOOTH_CHEBY || smoother > HPGMG_SMOOTH_JACOBI) return HPGMG_USER_BAD_ARGUMENT;
  if (!isfinite(a) || !isfinite(b) || a < 0.0 || !(b > 0.0)) return HPGMG_USER_BAD_ARGUMENT;
  if (!(h > 0.0) || !isfinite(h)) h = 1.0 / (double)n;
  const hpgmg_config cfg = { HPGMG_OP_7PT, smoother, a != 0.0, 1 };
  if (user_live > 0 && (cfg.smoother != user_cfg.smoother || cfg.helmholtz != user_cfg.helmholtz)) return HPGMG_USER_CONFLICT;
  if (hpgmg_configure(&cfg)) return HPGMG_USER_UNSUPPORTED;
  user_cfg = cfg;
  user_live++;

  hpgmg_user_solver *us = (hpgmg_user_solver *)calloc(1, sizeof(*us));
  hpgmg_solver *s = &us->s;
  us->n = n; us->bc = bc; us->operator_ok = us->rhs_ok = 1;
  us->max_iter = 100;
  us->mask = mask;
  USER_QUIET(us);
  s->boxes_in_i = n / box_dim; s->box_dim = box_dim; s->my_rank = 0; s->num_ranks = 1;
  s->a = a; s->b = b; s->h = h;
  us->x_id = hpgmg_vectors_reserved();
  create_level(&s->level_h, s->boxes_in_i, box_dim, stencil_get_radius(), us->x_id + 1, bc, 0, 1);
  s->level_h.h = h;
  { /* coefficients 1 (high domain faces included), f = 0: initialize_problem's layout with constant values */
    const size_t big = (size_t)n * n * (n + 1);
    double *ones = (double *)malloc(big * sizeof(double));
    size_t q;
    for (q = 0; q < big; q++) ones[q] = 1.0;
    if (mask) us->wall0 = hpgmg_vector_alloc((size_t)6 * n * n);
    user_pack_beta(us, VECTOR_BETA_I, ones, HPGMG_WHERE_HOST, HPGMG_DENSE_FACE_I);
    user_pack_beta(us, VECTOR_BETA_J, ones, HPGMG_WHERE_HOST, HPGMG_DENSE_FACE_J);
    user_pack_beta(us, VECTOR_BETA_K, ones, HPGMG_WHERE_HOST, HPGMG_DENSE_FACE_K);
    if (cfg.helmholtz) hpgmg_dense_pack(&s->level_h, VECTOR_ALPHA, ones, HPGMG_WHERE_HOST, HPGMG_DENSE_CELL, HPGMG_DENSE_CHECK_NONNEGATIVE);
    free(ones);
  }
  rebuild_operator(&s->level_h, NULL, a, b);
  /* six Neumann walls: a level of one cell would have Aii = 0 for Poisson, so stop at 2^3 as the periodic case does */
  MGBuild(&s->mg, &s->level_h, a, b, (bc == BC_PERIODIC || mask == 63) ? 2 : 1);
  if (mask) { user_bnd_alloc(us); user_walls_rebuilt(us); }
  USER_LOUD();
  *out = us;
  return HPGMG_USER_OK;
}

void hpgmg_user_destroy(hpgmg_user_solver *us) {
  if (!us) return;
  USER_QUIET(us);
  if (us->bnd_g) {
    int l;
    for (l = 0; l < us->s.mg.num_levels; l++) { hpgmg_vector_free(us->bnd_g[l]); hpgmg_vector_free(us->bnd_phi[l]); if (us->wall) hpgmg_vector_free(us->wall[l]); }
    hpgmg_vector_free(us->app_g); hpgmg_vector_free(us->app_phi);
    free(us->bnd_g); free(us->bnd_phi); free(us->wall);
  }
  MGDestroy(&us->s.mg);
  destroy_level(&us->s.level_h);     /* frees the plugin's staging buffer with the level */
  USER_LOUD();
  free(us);
  user_live--;
}

void hpgmg_user_set_verbose(hpgmg_user_solver *us, int on) { us->verbose = on; }
int hpgmg_user_set_max_iterations(hpgmg_user_solver *us, int n) {
  if (!us || n < 1) return HPGMG_USER_BAD_ARGUMENT;
  us->max_iter = n;
  return HPGMG_USER_OK;
}
hpgmg_solver *hpgmg_user_solver_of(hpgmg_user_solver *us) { return &us->s; }

int hpgmg_user_set_coefficients(hpgmg_user_solver *us, const double *alpha, const double *beta_i, const double *beta_j, const double *beta_k, int where) {
  hpgmg_solver *s = &us->s;
  level_type *L = &s->level_h;
  const int helmholtz = s->a != 0.0;
  if (!beta_i || !beta_j || !beta_k || (helmholtz && !alpha) || (!helmholtz && alpha)) return HPGMG_USER_BAD_ARGUMENT;
  if (!user_config_ok()) return HPGMG_USER_CONFLICT;
  int st = 0, e;
  USER_QUIET(us);
  us->operator_ok = 0;
  if (us->bnd) us->rhs_ok = 0;           /* the lifted f and every phi_l were made with the old beta: a new set_rhs_dirichlet is needed */
  if ((e = user_pack_beta(us, VECTOR_BETA_I, beta_i, where, HPGMG_DENSE_FACE_I)) < 0) goto refused;
  st |= e;
  if ((e = user_pack_beta(us, VECTOR_BETA_J, beta_j, where, HPGMG_DENSE_FACE_J)) < 0) goto refused;
  st |= e;
  if ((e = user_pack_beta(us, VECTOR_BETA_K, beta_k, where, HPGMG_DENSE_FACE_K)) < 0) goto refused;
  st |= e;
  if (helmholtz && (e = hpgmg_dense_pack(L, VECTOR_ALPHA, alpha, where, HPGMG_DENSE_CELL, HPGMG_DENSE_CHECK_NONNEGATIVE)) < 0) goto refused;
  if (helmholtz) st |= e;
  if (st) { USER_LOUD(); return user_pack_status(st); }
  rebuild_operator(L, NULL, s->a, s->b);
  MGRebuildCoarse(&s->mg, s->a, s->b);
  user_walls_rebuilt(us);
  us->operator_ok = 1;
  USER_LOUD();
  return HPGMG_USER_OK;
refused:
  USER_LOUD();
  return HPGMG_USER_BAD_ARGUMENT;
}

int hpgmg_user_set_rhs(hpgmg_user_solver *us, const double *f, int where, double *mean_shift) {
  level_type *L = &us->s.level_h;
  if (!f) return HPGMG_USER_BAD_ARGUMENT;
  if (us->mask) return hpgmg_user_set_rhs_dirichlet(us, f, NULL, where, mean_shift);     /* Neumann walls: zero data on every face, the F-cycle keeps its hook */
  USER_QUIET(us);
  const int st = user_pack_status(hpgmg_dense_pack(L, VECTOR_F, f, where, HPGMG_DENSE_CELL, HPGMG_DENSE_CHECK_FINITE));
  us->rhs_ok = (st == HPGMG_USER_OK);
  us->mean_shift = 0.0;
  us->bnd = 0;
  if (us->rhs_ok && L->must_subtract_mean) {     /* periodic without an a * alpha term: only a mean-free f has a solution (hpgmg_solver_create_explicit) */
    const double avg = mean(L, VECTOR_F);
    if (avg != 0.0) { shift_vector(L, VECTOR_F, VECTOR_F, -avg); us->mean_shift = avg; }
  }
  USER_LOUD();
  if (mean_shift) *mean_shift = us->mean_shift;
  return st;
}

/* boundary values: g_l and phi_l of every level, g and phi of apply_dirichlet -- 6 n_l^2 doubles each, allocated once */
static void user_bnd_alloc(hpgmg_user_solver *us) {
  const mg_type *G = &us->s.mg;
  int l;
  if (us->bnd_g) return;
  us->bnd_g = (double **)calloc((size_t)G->num_levels, sizeof(double *));
  us->bnd_phi = (double **)calloc((size_t)G->num_levels, sizeof(double *));
  if (us->mask) us->wall = (double **)calloc((size_t)G->num_levels, sizeof(double *));
  for (l = 0; l < G->num_levels; l++) {
    const size_t n = (size_t)G->levels[l]->dim.i;
    us->bnd_g[l] = hpgmg_vector_alloc(6 * n * n);
    us->bnd_phi[l] = hpgmg_vector_alloc(6 * n * n);
    if (us->mask) us->wall[l] = l ? hpgmg_vector_alloc(6 * n * n) : us->wall0;
  }
  us->app_g = hpgmg_vector_alloc((size_t)6 * us->n * us->n);
  us->app_phi = hpgmg_vector_alloc((size_t)6 * us->n * us->n);
}
static void user_bnd_take(hpgmg_user_solver *us, double *dst, const double *g, int where) {     /* the caller's g into plugin memory */
  const size_t len = (size_t)6 * us->n * us->n;
  if (where == HPGMG_WHERE_HOST) hpgmg_vector_upload(dst, g, len);
  else hpgmg_vector_copy(dst, g, len);
}

int hpgmg_user_set_rhs_dirichlet(hpgmg_user_solver *us, const double *f, const double *g, int where, double *mean_shift) {
  hpgmg_solver *s = &us->s;
  level_type *L = &s->level_h;
  int l;
  if (mean_shift) *mean_shift = 0.0;
  if (!f || (!g && !us->mask) || (where != HPGMG_WHERE_HOST && where != HPGMG_WHERE_PLUGIN)) return HPGMG_USER_BAD_ARGUMENT;
  if (us->bc != BC_DIRICHLET) return HPGMG_USER_UNSUPPORTED;
  USER_QUIET(us);
  user_bnd_alloc(us);
  us->bnd = 0; us->mean_shift = 0.0;
  if (g) user_bnd_take(us, us->bnd_g[0], g, where);
  else {                             /* a solver with Neumann walls and no data: zero on every face */
    double *zero = (double *)calloc((size_t)6 * us->n * us->n, sizeof(double));
    hpgmg_vector_upload(us->bnd_g[0], zero, (size_t)6 * us->n * us->n);
    free(zero);
  }
  const int st = user_pack_status(us->mask ? hpgmg_dense_pack_lifted_faces(L, VECTOR_F, f, where, us->bnd_g[0], s->b, us->mask, us->wall[0])
                                           : hpgmg_dense_pack_lifted(L, VECTOR_F, f, where, us->bnd_g[0], s->b));     /* F = f + T(g) */
  us->rhs_ok = (st == HPGMG_USER_OK);
  if (us->rhs_ok) {                  /* g_l and phi_l of every level, for the F-cycle's right-hand-side correction */
    for (l = 0; l < s->mg.num_levels; l++) {
      if (l > 0) hpgmg_boundary_restrict(s->mg.levels[l], us->bnd_g[l], s->mg.levels[l - 1], us->bnd_g[l - 1]);
      if (us->mask) hpgmg_boundary_flux_faces(s->mg.levels[l], us->bnd_phi[l], us->bnd_g[l], s->b, us->mask, us->wall[l]);
      else hpgmg_boundary_flux(s->mg.levels[l], us->bnd_phi[l], us->bnd_g[l], s->b);
    }
    us->bnd = 1;
    if (L->must_subtract_mean) {     /* six Neumann walls without an a * alpha term: only a mean-free f + T(g) has a solution */
      const double avg = mean(L, VECTOR_F);
      if (avg != 0.0) { shift_vector(L, VECTOR_F, VECTOR_F, -avg); us->mean_shift = avg; }
      if (mean_shift) *mean_shift = us->mean_shift;
    }
  }
  USER_LOUD();
  return st;
}

/* the F-cycle hook: R_l += T_l(g_l) - R_cell(T_{l-1}(g_{l-1})), so that R_l is the restricted f plus level l's own lift */
static void user_bnd_restricted(const hpgmg_fmg_hook *hook, mg_type *G, int l, int R_id) {
  const hpgmg_user_solver *us = (const hpgmg_user_solver *)hook->ctx;
  hpgmg_boundary_lift(G->levels[l], R_id, us->bnd_phi[l], us->bnd_phi[l - 1], 1.0);
}
/* after interpolation_fcycle onto level l: the fine cells that read a coarse ghost get what the inhomogeneous ghost adds */
static void user_bnd_interpolated(const hpgmg_fmg_hook *hook, mg_type *G, int l, int e_id) {
  const hpgmg_user_solver *us = (const hpgmg_user_solver *)hook->ctx;
  if (us->mask) hpgmg_boundary_interp_faces(G->levels[l], e_id, G->levels[l + 1], us->bnd_g[l + 1], us->mask);
  else hpgmg_boundary_interp(G->levels[l], e_id, G->levels[l + 1], us->bnd_g[l + 1]);
}

int hpgmg_user_solve(hpgmg_user_solver *us, int method, double rtol, const double *u0, int where, hpgmg_user_info *info) {
  hpgmg_solver *s = &us->s;
  level_type *L = &s->level_h;
  if ((method != HPGMG_USER_FMG && method != HPGMG_USER_MG && method != HPGMG_USER_PCG && method != HPGMG_USER_FPCG) || !(rtol > 0.0)) return HPGMG_USER_BAD_ARGUMENT;
  if (!us->operator_ok || !us->rhs_ok) return HPGMG_USER_NOT_READY;
  if (!user_config_ok()) return HPGMG_USER_CONFLICT;
  USER_QUIET(us);
  const int v0 = L->vcycles_from_this_level;
  double norm_of_F, r;
  if (method == HPGMG_USER_PCG || method == HPGMG_USER_FPCG) {    /* CG around the V-cycle, from u0 or from 0 */
    if (u0) {
      const int st = user_pack_status(hpgmg_dense_pack(L, VECTOR_U, u0, where, HPGMG_DENSE_CELL, HPGMG_DENSE_CHECK_FINITE));
      if (st) { USER_LOUD(); return st; }
    }
    (method == HPGMG_USER_FPCG ? MGFPCGSolve : MGPCGSolve)(&s->mg, 0, VECTOR_U, VECTOR_F, s->a, s->b, rtol, us->max_iter, u0 != NULL);
    norm_of_F = hpgmg_last_solve.norm_of_F; r = hpgmg_last_solve.norm_of_residual;
  } else
  if (u0) {                     /* u = u0 + e with A e = f - A u0; the V-cycles stop when |f - A u| has dropped below rtol |f| */
    const int st = user_pack_status(hpgmg_dense_pack(L, VECTOR_U, u0, where, HPGMG_DENSE_CELL, HPGMG_DENSE_CHECK_FINITE));
    if (st) { USER_LOUD(); return st; }
    residual(L, us->x_id, VECTOR_U, VECTOR_F, s->a, s->b);
    norm_of_F = norm(L, VECTOR_F);
    const double norm_of_r0 = norm(L, us->x_id);
    if (norm_of_r0 > 0.0) {
      MGSolve(&s->mg, 0, VECTOR_U, us->x_id, s->a, s->b, rtol * norm_of_F / norm_of_r0);
      hpgmg_dense_pack(L, us->x_id, u0, where, HPGMG_DENSE_CELL, HPGMG_DENSE_CHECK_FINITE);
      add_vectors(L, VECTOR_U, 1.0, VECTOR_U, 1.0, us->x_id);
    }
    residual(L, VECTOR_TEMP, VECTOR_U, VECTOR_F, s->a, s->b);
    r = norm(L, VECTOR_TEMP);
  } else if (method == HPGMG_USER_FMG) {           /* the benchmark's solve (hpgmg_solver_fmg) */
    hpgmg_fmg_hook hook = { user_bnd_restricted, user_bnd_interpolated, us, 0 };
    hook.key = 1 + (long long)(uintptr_t)us->bnd_phi;
    if (us->bnd) hpgmg_fmg_set_hook(&hook);
    hpgmg_fmg_zero_u_first();
    FMGSolve(&s->mg, 0, VECTOR_U, VECTOR_F, s->a, s->b, rtol);
    hpgmg_fmg_set_hook(NULL);
    norm_of_F = hpgmg_last_solve.norm_of_F; r = hpgmg_last_solve.norm_of_residual;
  } else {
    MGSolve(&s->mg, 0, VECTOR_U, VECTOR_F, s->a, s->b, rtol);
    norm_of_F = hpgmg_last_solve.norm_of_F; r = hpgmg_last_solve.norm_of_residual;
  }
  USER_LOUD();
  if (info) {
    info->norm_of_residual = r; info->norm_of_f = norm_of_F; info->mean_shift = us->mean_shift;
    info->vcycles = L->vcycles_from_this_level - v0;
    info->converged = (r == 0.0) || (r < rtol * norm_of_F);
  }
  return HPGMG_USER_OK;
}

int hpgmg_user_get_solution(hpgmg_user_solver *us, double *u, int where) {
  USER_QUIET(us);
  const int st = hpgmg_dense_unpack(&us->s.level_h, VECTOR_U, u, where);
  USER_LOUD();
  return st < 0 ? HPGMG_USER_BAD_ARGUMENT : HPGMG_USER_OK;
}

int hpgmg_user_apply(hpgmg_user_solver *us, const double *x, double *y, int where) {
  hpgmg_solver *s = &us->s;
  level_type *L = &s->level_h;
  if (!y) return HPGMG_USER_BAD_ARGUMENT;
  if (!us->operator_ok) return HPGMG_USER_NOT_READY;
  if (!user_config_ok()) return HPGMG_USER_CONFLICT;
  USER_QUIET(us);
  int st = user_pack_status(hpgmg_dense_pack(L, us->x_id, x, where, HPGMG_DENSE_CELL, HPGMG_DENSE_CHECK_FINITE));
  if (st == HPGMG_USER_OK) {
    apply_op(L, VECTOR_R, us->x_id, s->a, s->b);      /* VECTOR_R: every solve sets it from f before reading it */
    if (hpgmg_dense_unpack(L, VECTOR_R, y, where) < 0) st = HPGMG_USER_BAD_ARGUMENT;
  }
  USER_LOUD();
  return st;
}

int hpgmg_user_apply_dirichlet(hpgmg_user_solver *us, const double *x, const double *g, double *y, int where) {
  hpgmg_solver *s = &us->s;
  level_type *L = &s->level_h;
  if (!x || !g || !y || (where != HPGMG_WHERE_HOST && where != HPGMG_WHERE_PLUGIN)) return HPGMG_USER_BAD_ARGUMENT;
  if (us->bc != BC_DIRICHLET) return HPGMG_USER_UNSUPPORTED;
  if (!us->operator_ok) return HPGMG_USER_NOT_READY;
  if (!user_config_ok()) return HPGMG_USER_CONFLICT;
  USER_QUIET(us);
  user_bnd_alloc(us);
  user_bnd_take(us, us->app_g, g, where);
  int st = user_pack_status(us->mask ? hpgmg_boundary_flux_faces(L, us->app_phi, us->app_g, s->b, us->mask, us->wall[0])
                                     : hpgmg_boundary_flux(L, us->app_phi, us->app_g, s->b));
  if (st == HPGMG_USER_OK) st = user_pack_status(hpgmg_dense_pack(L, us->x_id, x, where, HPGMG_DENSE_CELL, HPGMG_DENSE_CHECK_FINITE));
  if (st == HPGMG_USER_OK) {
    apply_op(L, VECTOR_R, us->x_id, s->a, s->b);
    hpgmg_boundary_lift(L, VECTOR_R, us->app_phi, NULL, -1.0);    /* y = A0 x - T(g) */
    if (hpgmg_dense_unpack(L, VECTOR_R, y, where) < 0) st = HPGMG_USER_BAD_ARGUMENT;
  }
  USER_LOUD();
  return st;
}

/* ------------------------------------------------------------------ CLI */
static int usage(int rank) {
  if (rank == 0) fprintf(stderr,
    "usage: hpgmg-fv [--op 7pt|27pt|fv4|fv2] [--smoother cheby|gsrb|jacobi] [--helmholtz] [--const-coeff] [--fp32-smoother] [--periodic] [--bottom-solver bicgstab|cg|cabicgstab|cacg]\n"
    "                [--vcycles] [--ucycles] [--unlimit] [--mgpcg]\n"
    "                [--warmup N] [--solves N] [--rank R --ranks N]  log2_box_dim  target_boxes_per_rank\n");
  return 0;
}

int hpgmg_fv_main(int argc, char **argv) {
  hpgmg_config cfg = { HPGMG_OP_7PT, HPGMG_SMOOTH_CHEBY, 0, 1 };
  int bc = BC_DIRICHLET;
  int pos[2], npos = 0, a, my_rank = 0, num_ranks = 1, warmup = 10, solves = 10, test_error_only = 0, mgpcg = 0;
  const hpgmg_transport *T = hpgmg_get_transport();
  if (T) { my_rank = T->rank; num_ranks = T->size; }
  for (a = 1; a < argc; a++) {
    if (!strcmp(argv[a], "--op") && a + 1 < argc) { a++;
      if (!strcmp(argv[a], "7pt")) cfg.op = HPGMG_OP_7PT; else if (!strcmp(argv[a], "27pt")) { cfg.op = HPGMG_OP_27PT; cfg.variable_coeff = 0; }
      else if (!strcmp(argv[a], "fv4")) cfg.op = HPGMG_OP_FV4; else if (!strcmp(argv[a], "fv2")) cfg.op = HPGMG_OP_FV2; else return usage(my_rank);
    } else if (!strcmp(argv[a], "--smoother") && a + 1 < argc) { a++;
      if (!strcmp(argv[a], "cheby")) cfg.smoother = HPGMG_SMOOTH_CHEBY; else if (!strcmp(argv[a], "gsrb")) cfg.smoother = HPGMG_SMOOTH_GSRB;
      else if (!strcmp(argv[a], "jacobi")) cfg.smoother = HPGMG_SMOOTH_JACOBI; else return usage(my_rank);
    } else if (!strcmp(argv[a], "--helmholtz")) cfg.helmholtz = 1;
    else if (!strcmp(argv[a], "--const-coeff")) cfg.variable_coeff = 0;
    else if (!strcmp(argv[a], "--fp32-smoother")) hpgmg_set_smoother_precision(32);
    else if (!strcmp(argv[a], "--periodic")) bc = BC_PERIODIC;                       /* the reference's -DUSE_PERIODIC_BC */
    else if (!strcmp(argv[a], "--test-error")) test_error_only = 1;
    else if (!strcmp(argv[a], "--bottom-solver") && a + 1 < argc) { a++;              /* the reference's -DUSE_BICGSTAB (default) / -DUSE_CG / -DUSE_CABICGSTAB / -DUSE_CACG */
      if (!strcmp(argv[a], "cg")) hpgmg_set_bottom_solver(HPGMG_BOTTOM_CG); else if (!strcmp(argv[a], "bicgstab")) hpgmg_set_bottom_solver(HPGMG_BOTTOM_BICGSTAB);
      else if (!strcmp(argv[a], "cabicgstab")) hpgmg_set_bottom_solver(HPGMG_BOTTOM_CABICGSTAB); else if (!strcmp(argv[a], "cacg")) hpgmg_set_bottom_solver(HPGMG_BOTTOM_CACG);
      else return usage(my_rank);
    }
    else if (!strcmp(argv[a], "--vcycles")) solve_with_vcycles = 1;
    else if (!strcmp(argv[a], "--ucycles")) hpgmg_set_ucycles(1);                    /* the reference's -DUSE_UCYCLES: no agglomeration */
    else if (!strcmp(argv[a], "--unlimit")) hpgmg_set_fmg_vcycles(20);               /* the reference's -DUNLIMIT_FMG_ITERATIONS */
    else if (!strcmp(argv[a], "--mgpcg")) mgpcg = 1;                                 /* the reference's third driver (mg.c:1500), which its main() never calls: two solves, then exit */
    else if (!strcmp(argv[a], "--warmup") && a + 1 < argc) warmup = atoi(argv[++a]);
    else if (!strcmp(argv[a], "--solves") && a + 1 < argc) solves = atoi(argv[++a]);
    else if (npos < 2 && argv[a][0] != '-') pos[npos++] = atoi(argv[a]);
    else return usage(my_rank);
  }
  if (npos != 2) return usage(my_rank);
  if (pos[0] > 9) { if (my_rank == 0) fprintf(stderr, "log2_box_dim must be less than 10\n"); return 0; }
  if (pos[0] < 4) { if (my_rank == 0) fprintf(stderr, "log2_box_dim must be at least 4\n"); return 0; }
  if (pos[1] < 1) { if (my_rank == 0) fprintf(stderr, "target_boxes_per_rank must be at least 1\n"); return 0; }
  if (hpgmg_configure(&cfg)) { if (my_rank == 0) fprintf(stderr, "unsupported operator/smoother combination\n"); return 1; }

  SAY(my_rank, "\n\n********************************************************************************\n"
               "***                            HPGMG-FV Benchmark                            ***\n"
               "********************************************************************************\n");
  SAY(my_rank, "%d MPI Tasks of %d threads   [backend: %s]\n", num_ranks, host_threads(), hpgmg_backend_name());
  SAY(my_rank, "\n\n===== Benchmark setup ==========================================================\n");

  hpgmg_solver *s = hpgmg_solver_create(pos[0], pos[1], bc, my_rank, num_ranks);
  if (!s) return 0;

  enum { DYNAMIC_RANGE = 3 };
  double avg[DYNAMIC_RANGE];
  int l, n;
  if (mgpcg) {                     /* what oracle/mgpcg_harness.c prints around the reference's MGPCG */
    level_type *L0 = s->mg.levels[0];
    for (n = 0; n < 2; n++) {
      MGPCG(&s->mg, 0, VECTOR_U, VECTOR_F, s->a, s->b, 1e-10);
      SAY(my_rank, "MGPCG solve %d: norm(u)=%1.15e  Krylov iterations on the fine level so far=%d\n", n, norm(L0, VECTOR_U), L0->Krylov_iterations);
    }
    const double uf = dot(L0, VECTOR_U, VECTOR_F), mu = mean(L0, VECTOR_U);
    SAY(my_rank, "MGPCG dot(u,f)=%1.15e  mean(u)=%1.15e\n", uf, mu);
    hpgmg_solver_destroy(s);
    return 0;
  }
  if (!test_error_only) {
    for (l = 0; l < DYNAMIC_RANGE; l++) {
      hpgmg_solver_restrict_rhs(s, l);
      SAY(my_rank, "\n\n===== Warming up by running %d solves ==========================================\n", warmup);
      MGResetTimers(&s->mg);
      for (n = 0; n < warmup; n++) hpgmg_solver_fmg(s, l);
      SAY(my_rank, "\n\n===== Running %d solves ========================================================\n", solves);
      MGResetTimers(&s->mg);
      for (n = 0; n < solves; n++) hpgmg_solver_fmg(s, l);
      avg[l] = s->mg.timers.MGSolve / (double)s->mg.MGSolves_performed;
      /* The table must hold DEVICE time per operator (launches are asynchronous), but a hipEvent pair around every operator
       * slows a solve by ~40 %: so the performance figures above come from the uninstrumented solves, and the table from a few
       * extra, silent, instrumented ones (HPGMG_TIMERS=host|device|sync picks one mode for everything instead). */
      if (!strcmp(hpgmg_backend_name(), "hip") && hpgmg_get_timer_mode() == 0 && !getenv("HPGMG_TIMERS")) {
        const int quiet = hpgmg_verbose, extra = solves < 5 ? solves : 5;
        hpgmg_set_timer_mode(1);
        MGResetTimers(&s->mg);
        hpgmg_verbose = 0;
        for (n = 0; n < extra; n++) hpgmg_solver_fmg(s, l);
        hpgmg_verbose = quiet;
        hpgmg_timers_settle();
        hpgmg_set_timer_mode(0);
      }
      SAY(my_rank, "\n\n===== Timing Breakdown =========================================================\n");
      MGPrintTiming(&s->mg, l);
    }
    SAY(my_rank, "\n\n===== Performance Summary ======================================================\n");
    for (l = 0; l < DYNAMIC_RANGE; l++) {
      level_type *L = s->mg.levels[l];
      double dof = (double)L->dim.i * (double)L->dim.j * (double)L->dim.k;
      SAY(my_rank, "  h=%0.15e  DOF=%0.15e  time=%0.6f  DOF/s=%0.3e  MPI=%d  OMP=%d\n", L->h, dof, avg[l], dof / avg[l], num_ranks, host_threads());
    }
  }
  SAY(my_rank, "\n\n===== Richardson error analysis ================================================\n");
  { double out[2]; hpgmg_solver_richardson(s, out); }
  SAY(my_rank, "\n\n===== Deallocating memory ======================================================\n");
  hpgmg_solver_destroy(s);
  SAY(my_rank, "\n\n===== Done =====================================================================\n");
  (void)now;
  return 0;
}

/* ------------------------------------------------------------------ accessors */
void hpgmg_level_info(const level_type *L, int out[HPGMG_INFO_COUNT]) {
  out[HPGMG_INFO_DIM] = L->dim.i;            out[HPGMG_INFO_BOX_DIM] = L->box_dim;
  out[HPGMG_INFO_GHOSTS] = L->box_ghosts;    out[HPGMG_INFO_JSTRIDE] = L->box_jStride;
  out[HPGMG_INFO_KSTRIDE] = L->box_kStride;  out[HPGMG_INFO_VOLUME] = L->box_volume;
  out[HPGMG_INFO_NUM_MY_BOXES] = L->num_my_boxes; out[HPGMG_INFO_NUM_VECTORS] = L->numVectors;
  out[HPGMG_INFO_BOXES_IN_I] = L->boxes_in.i; out[HPGMG_INFO_MY_RANK] = L->my_rank;
  out[HPGMG_INFO_NUM_RANKS] = L->num_ranks;  out[HPGMG_INFO_NUM_MY_BLOCKS] = L->num_my_blocks;
  out[HPGMG_INFO_ACTIVE] = L->active;
}
/* per-level timing table row values (seconds accumulated since MGResetTimers), after settling pending device timers:
 * out[0..7] = smooth, residual, apply_op, blas1, boundary_conditions, restriction_total, interpolation_total, ghostZone_total; out[8] = Total */
void hpgmg_level_timers(level_type *L, double out[9]) {
  hpgmg_level_sync_counters(L);
  out[0] = L->timers.smooth; out[1] = L->timers.residual; out[2] = L->timers.apply_op; out[3] = L->timers.blas1;
  out[4] = L->timers.boundary_conditions; out[5] = L->timers.restriction_total; out[6] = L->timers.interpolation_total;
  out[7] = L->timers.ghostZone_total; out[8] = L->timers.Total;
}
double hpgmg_level_h(const level_type *L) { return L->h; }
double hpgmg_level_eigenvalue(const level_type *L) { return L->dominant_eigenvalue_of_DinvA; }
void hpgmg_level_set_eigenvalue(level_type *L, double v) { L->dominant_eigenvalue_of_DinvA = v; }
void hpgmg_level_box_low(const level_type *L, int box, int out[3]) {
  out[0] = L->my_boxes[box].low.i; out[1] = L->my_boxes[box].low.j; out[2] = L->my_boxes[box].low.k;
}
/* which: 0 exchange_ghosts[shape], 1 restriction[type], 2 interpolation, 3 boundary_condition[shape] (out[0] only) */
int hpgmg_level_list_counts(const level_type *L, int which, int idx, int out[3]) {
  const communicator_type *C = NULL;
  out[0] = out[1] = out[2] = 0;
  if (which == 0) C = &L->exchange_ghosts[idx]; else if (which == 1) C = &L->restriction[idx]; else if (which == 2) C = &L->interpolation;
  else { out[0] = L->boundary_condition.num_blocks[idx]; return 0; }
  out[0] = C->num_blocks[0]; out[1] = C->num_blocks[1]; out[2] = C->num_blocks[2];
  return C->num_sends + C->num_recvs;
}
void hpgmg_level_read_vector(level_type *L, int box, int id, double *host_out) {
  hpgmg_vector_download(host_out, L->my_boxes[box].vectors[id], (size_t)L->box_volume);
}
void hpgmg_level_write_vector(level_type *L, int box, int id, const double *host_in) {
  hpgmg_vector_upload(L->my_boxes[box].vectors[id], host_in, (size_t)L->box_volume);
}
level_type *hpgmg_level_create(int boxes_in_i, int box_dim, int ghosts, int numVectors, int bc, int my_rank, int num_ranks, double h) {
  level_type *L = (level_type *)malloc(sizeof(level_type));
  create_level(L, boxes_in_i, box_dim, ghosts, numVectors, bc, my_rank, num_ranks);
  L->h = h;
  return L;
}
void hpgmg_level_destroy(level_type *L) { if (L) { destroy_level(L); free(L); } }
mg_type *hpgmg_mg_create(level_type *fine, double a, double b, int minCoarseDim) {
  mg_type *G = (mg_type *)calloc(1, sizeof(mg_type));
  MGBuild(G, fine, a, b, minCoarseDim);
  return G;
}
void hpgmg_mg_destroy(mg_type *G) { if (G) { MGDestroy(G); free(G); } }
level_type *hpgmg_mg_level(mg_type *G, int l) { return (l >= 0 && l < G->num_levels) ? G->levels[l] : NULL; }
int hpgmg_mg_num_levels(const mg_type *G) { return G->num_levels; }
