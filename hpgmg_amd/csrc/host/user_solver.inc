/*
 * user_solver.inc -- user problems on dense arrays (include/hpgmg_fv.h hpgmg_user_*): a 7-point variable-coefficient solver whose coefficients,
 * right-hand side and boundary values come from the caller's arrays, around the hierarchy of host/mg.c.  It reaches the arrays through the
 * dense-array and boundary hooks of include/hpgmg_operators.h (host defaults: host/hooks_host.inc; HIP: host/plugin_dense.c, host/plugin_pcg.c, host/plugin_step.c).
 * DESIGN.md §11.  A part of host/driver.c's translation unit, included there.
 */
#include <stdlib.h>
#include <math.h>
#include <stdint.h>
#include "hpgmg_fv.h"

struct hpgmg_user_solver {
  hpgmg_solver s;              /* the finest level, the hierarchy, a, b, h */
  int n, bc, verbose;
  int x_id;                    /* the finest level's one extra vector: u0 of a warm start, the operand of apply */
  int operator_ok, rhs_ok;     /* 0 after a set_coefficients / set_rhs that was refused part way */
  int coef_given;              /* 1 once a set_coefficients succeeded (until then the coefficients are create's ones: sensitivity has no arrays to differentiate) */
  double mean_shift;           /* what the last set_rhs subtracted from f */
  int bnd;                     /* 1: f was set with boundary values (set_rhs_dirichlet): an F-cycle runs with the hook below */
  double **bnd_g, **bnd_phi;   /* per level: the boundary values g_l and their lift flux phi_l (plugin memory; allocated on first use) */
  double *app_g, *app_phi;     /* apply_dirichlet's g and phi on the finest level */
  int max_iter;                /* HPGMG_USER_PCG / _FPCG: the iteration limit (hpgmg_user_set_max_iterations; default 100) */
  int mask;                    /* bit f: domain face f is a Neumann or Robin wall (hpgmg_user_create_faces; DESIGN.md §11.2, §11.5); 0: every wall Dirichlet, or periodic */
  double *wall0, **wall;       /* mask != 0: wall0 = wall[0]; per level, the wall beta of the masked faces (a boundary array; the level's own beta is 0 there,
                                  on a Robin wall wall * t / (2 + t)) */
  int robin_mask;              /* bit f: face f is a Robin wall (a subset of mask) */
  int kappa_positive;          /* some kappa of a Robin face is > 0: six masked walls are then not singular */
  double **kappa;              /* robin_mask != 0: per level, kappa of the Robin walls (a boundary array, 0.0 on the other faces), allocated and freed with wall */
  int march;                   /* 1: a theta march is live (hpgmg_user_start; DESIGN.md §11.8): VECTOR_U holds its state u, w_id its rate w = alpha du/dt;
                                  2: a wave march is (hpgmg_user_wave_start, host/user_wave.inc; DESIGN.md §11.12): w_id holds v = du/dt, q_id the acceleration */
  int uold_id, w_id;           /* the finest level's two vectors of a march (0 until the first hpgmg_user_start / _wave_start creates them) */
  int q_id;                    /* and the wave march's third (0 until the first hpgmg_user_wave_start) */
  double dt, theta;            /* of the last start / step (dt: of either march) */
  double wave_beta, wave_gamma, wave_sigma, wave_t;      /* of the last wave_start; the time since it */
  int eig_n, eig_ids[6 * HPGMG_USER_EIGS_MAX_BLOCK];      /* the finest level's vectors of hpgmg_user_eigs (host/user_eigs.inc), in the order they were created */
};
static int user_live = 0;              /* user solvers alive: the process-wide configuration belongs to them */
static hpgmg_config user_cfg;

/* user calls print only when the solver's verbose flag is on (the library's default, hpgmg_verbose = 1, is the benchmark's) */
#define USER_QUIET(us) const int verbose_saved_ = hpgmg_verbose; hpgmg_verbose = (us)->verbose
#define USER_LOUD() hpgmg_verbose = verbose_saved_
#define USER_KAPPA(us, l) ((us)->kappa ? (us)->kappa[l] : NULL)      /* level l's kappa array; NULL: no Robin wall, the _faces forms */

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
static void user_bnd_take(hpgmg_user_solver *us, double *dst, const double *g, int where);
/* a face array of the coefficients into the finest level: with Neumann walls through the masked pack, which keeps their beta in wall[0] */
static int user_pack_beta(hpgmg_user_solver *us, int id, const double *src, int where, int layout) {
  level_type *L = &us->s.level_h;
  if (!us->mask) return hpgmg_dense_pack(L, id, src, where, layout, HPGMG_DENSE_CHECK_POSITIVE);
  return hpgmg_dense_pack_walls(L, id, src, where, layout, HPGMG_DENSE_CHECK_POSITIVE, us->mask, us->wall0);
}
/* after rebuild_operator + MGRebuildCoarse of a solver with Neumann walls: every level's wall beta, and the singular case.  Six Neumann walls
 * without an a * alpha term leave the constants in the null space, as periodic Poisson does: the same path (MGRebuildCoarse has just reset it) */
static void user_walls_rebuilt(hpgmg_user_solver *us, int restricted) {      /* restricted: MGRebuildCoarseWalls has made wall[l] already */
  mg_type *G = &us->s.mg;
  int l;
  if (!us->mask) return;
  if (!restricted) for (l = 1; l < G->num_levels; l++) hpgmg_boundary_restrict(G->levels[l], us->wall[l], G->levels[l - 1], us->wall[l - 1]);
  if (us->mask != 63 || us->kappa_positive) return;
  for (l = 0; l < G->num_levels; l++) {
    level_type *L = G->levels[l];
    int alpha_is_zero = 1;
    if (hpgmg_vectors_reserved() > VECTOR_ALPHA && L->active) alpha_is_zero = (dot(L, VECTOR_ALPHA, VECTOR_ALPHA) == 0.0);
    if (us->s.a == 0 || alpha_is_zero) L->must_subtract_mean = 1;
  }
}

/* MGRebuildCoarseWalls' callback of a solver with a Robin wall (DESIGN.md §11.5): level l's wall beta and kappa from level l - 1's, then the
 * level's beta on the masked walls from them and its own h */
static void user_store_walls(void *ctx, mg_type *G, int l) {
  hpgmg_user_solver *us = (hpgmg_user_solver *)ctx;
  hpgmg_boundary_restrict(G->levels[l], us->wall[l], G->levels[l - 1], us->wall[l - 1]);
  hpgmg_boundary_restrict(G->levels[l], us->kappa[l], G->levels[l - 1], us->kappa[l - 1]);
  hpgmg_boundary_store_walls(G->levels[l], us->wall[l], us->kappa[l], us->mask);
}

/* every level's operator from the finest level's coefficient vectors (and wall[0], kappa[0]) with the solver's a, b: what follows the packs of
 * set_coefficients, and all of set_shift */
static void user_rebuild(hpgmg_user_solver *us) {
  hpgmg_solver *s = &us->s;
  level_type *L = &s->level_h;
  if (us->robin_mask) {                  /* the wall's part of the diagonal depends on each level's own h (DESIGN.md §11.5) */
    hpgmg_boundary_store_walls(L, us->wall[0], us->kappa[0], us->mask);
    rebuild_operator(L, NULL, s->a, s->b);
    MGRebuildCoarseWalls(&s->mg, s->a, s->b, user_store_walls, us);
  } else {
    rebuild_operator(L, NULL, s->a, s->b);
    MGRebuildCoarse(&s->mg, s->a, s->b);
  }
  user_walls_rebuilt(us, us->robin_mask != 0);
}

static int user_create(int n, int box_dim, int bc, int mask, int robin_mask, int op, int smoother, double a, double b, double h, hpgmg_user_solver **out);
int hpgmg_user_create(int n, int box_dim, int bc, int op, int smoother, double a, double b, double h, hpgmg_user_solver **out) {
  return user_create(n, box_dim, bc, 0, 0, op, smoother, a, b, h, out);
}
int hpgmg_user_create_faces(int n, int box_dim, const int face_bc[6], int op, int smoother, double a, double b, double h, hpgmg_user_solver **out) {
  int f, mask = 0, robin_mask = 0;
  if (out) *out = NULL;
  if (!face_bc) return HPGMG_USER_BAD_ARGUMENT;
  for (f = 0; f < 6; f++) {
    if (face_bc[f] != HPGMG_FACE_DIRICHLET && face_bc[f] != HPGMG_FACE_NEUMANN && face_bc[f] != HPGMG_FACE_ROBIN) return HPGMG_USER_BAD_ARGUMENT;
    if (face_bc[f] != HPGMG_FACE_DIRICHLET) mask |= 1 << f;
    if (face_bc[f] == HPGMG_FACE_ROBIN) robin_mask |= 1 << f;
  }
  return user_create(n, box_dim, BC_DIRICHLET, mask, robin_mask, op, smoother, a, b, h, out);       /* mask 0 is hpgmg_user_create's solver */
}

static int user_create(int n, int box_dim, int bc, int mask, int robin_mask, int op, int smoother, double a, double b, double h, hpgmg_user_solver **out) {
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
  us->mask = mask; us->robin_mask = robin_mask;      /* kappa starts as 0: Neumann walls until set_coefficients_robin */
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
  if (mask) { user_bnd_alloc(us); user_walls_rebuilt(us, 0); }
  USER_LOUD();
  *out = us;
  return HPGMG_USER_OK;
}

void hpgmg_user_destroy(hpgmg_user_solver *us) {
  if (!us) return;
  USER_QUIET(us);
  if (us->bnd_g) {
    int l;
    for (l = 0; l < us->s.mg.num_levels; l++) {
      hpgmg_vector_free(us->bnd_g[l]); hpgmg_vector_free(us->bnd_phi[l]);
      if (us->wall) hpgmg_vector_free(us->wall[l]);
      if (us->kappa) hpgmg_vector_free(us->kappa[l]);
    }
    hpgmg_vector_free(us->app_g); hpgmg_vector_free(us->app_phi);
    free(us->bnd_g); free(us->bnd_phi); free(us->wall); free(us->kappa);
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

/* kappa of set_coefficients_robin into kappa[0]: validated as the caller gave it, then 0.0 on the faces that are not Robin */
static int user_take_kappa(hpgmg_user_solver *us, const double *kappa, int where) {
  const size_t face = (size_t)us->n * us->n;
  int f, st;
  user_bnd_take(us, us->kappa[0], kappa, where);
  st = hpgmg_boundary_check_kappa(&us->s.level_h, us->kappa[0], HPGMG_WHERE_PLUGIN, us->robin_mask, &us->kappa_positive);
  if (us->robin_mask != 63) {
    double *zero = (double *)calloc(face, sizeof(double));
    for (f = 0; f < 6; f++) if (!((us->robin_mask >> f) & 1)) hpgmg_vector_upload(us->kappa[0] + f * face, zero, face);
    free(zero);
  }
  return st;
}

int hpgmg_user_set_coefficients(hpgmg_user_solver *us, const double *alpha, const double *beta_i, const double *beta_j, const double *beta_k, int where) {
  if (us->robin_mask) return HPGMG_USER_BAD_ARGUMENT;      /* a Robin wall needs its kappa: hpgmg_user_set_coefficients_robin */
  return hpgmg_user_set_coefficients_robin(us, alpha, beta_i, beta_j, beta_k, NULL, where);
}

/* What set_coefficients_robin and set_cell_coefficients share.  user_coef_begin: the alpha / a and kappa / robin_mask rules and the configuration; then
 * the operator, a live march and a lifted right-hand side are invalid, and kappa is taken.  HPGMG_USER_OK: go on and pack (under USER_QUIET, which the
 * caller holds); anything else is the call's result.  user_coef_end: st the packs' status bits so far (< 0: one was refused); alpha last, then every
 * level's operator. */
static int user_coef_begin(hpgmg_user_solver *us, const double *alpha, const double *kappa, int where) {
  const int helmholtz = us->s.a != 0.0;
  int e;
  if ((helmholtz && !alpha) || (!helmholtz && alpha)) return HPGMG_USER_BAD_ARGUMENT;
  if ((us->robin_mask != 0) != (kappa != NULL)) return HPGMG_USER_BAD_ARGUMENT;
  if (kappa && where != HPGMG_WHERE_HOST && where != HPGMG_WHERE_PLUGIN) return HPGMG_USER_BAD_ARGUMENT;
  if (!user_config_ok()) return HPGMG_USER_CONFLICT;
  us->operator_ok = 0;
  us->march = 0;
  if (us->bnd) us->rhs_ok = 0;           /* the lifted f and every phi_l were made with the old beta: a new set_rhs_dirichlet is needed */
  if (kappa && (e = user_take_kappa(us, kappa, where)) != 0) return user_pack_status(e);
  return HPGMG_USER_OK;
}
static int user_coef_end(hpgmg_user_solver *us, const double *alpha, int where, int st) {
  int e;
  if (st < 0) return HPGMG_USER_BAD_ARGUMENT;
  if (us->s.a != 0.0) {
    if ((e = hpgmg_dense_pack(&us->s.level_h, VECTOR_ALPHA, alpha, where, HPGMG_DENSE_CELL, HPGMG_DENSE_CHECK_NONNEGATIVE)) < 0) return HPGMG_USER_BAD_ARGUMENT;
    st |= e;
  }
  if (st) return user_pack_status(st);
  user_rebuild(us);
  us->operator_ok = us->coef_given = 1;
  return HPGMG_USER_OK;
}

int hpgmg_user_set_coefficients_robin(hpgmg_user_solver *us, const double *alpha, const double *beta_i, const double *beta_j, const double *beta_k,
                                      const double *kappa, int where) {
  if (!beta_i || !beta_j || !beta_k) return HPGMG_USER_BAD_ARGUMENT;
  USER_QUIET(us);
  int st = user_coef_begin(us, alpha, kappa, where), e;
  if (st == HPGMG_USER_OK) {
    if ((e = user_pack_beta(us, VECTOR_BETA_I, beta_i, where, HPGMG_DENSE_FACE_I)) >= 0) st |= e;
    if (e >= 0 && (e = user_pack_beta(us, VECTOR_BETA_J, beta_j, where, HPGMG_DENSE_FACE_J)) >= 0) st |= e;
    if (e >= 0 && (e = user_pack_beta(us, VECTOR_BETA_K, beta_k, where, HPGMG_DENSE_FACE_K)) >= 0) st |= e;
    st = user_coef_end(us, alpha, where, e < 0 ? -1 : st);
  }
  USER_LOUD();
  return st;
}

/* cell-centred conductivities (DESIGN.md §11.10): set_coefficients_robin with the three packs replaced by the one of the cell-mean hook */
int hpgmg_user_set_cell_coefficients(hpgmg_user_solver *us, const double *alpha, const double *kcell, int mean, const double *kappa, int where) {
  if (!us || !kcell || (mean != HPGMG_MEAN_HARMONIC && mean != HPGMG_MEAN_ARITHMETIC)) return HPGMG_USER_BAD_ARGUMENT;
  USER_QUIET(us);
  int st = user_coef_begin(us, alpha, kappa, where);
  if (st == HPGMG_USER_OK) st = user_coef_end(us, alpha, where, hpgmg_dense_pack_cell_mean(&us->s.level_h, kcell, where, mean, us->mask, us->wall0));
  USER_LOUD();
  return st;
}

/* the bodies of set_rhs / set_rhs_dirichlet: a march packs its F = f + T(g) through them too, and goes on (DESIGN.md §11.8) */
static int user_rhs_lifted(hpgmg_user_solver *us, const double *f, const double *g, int where, double *mean_shift);
static int user_rhs_plain(hpgmg_user_solver *us, const double *f, int where, double *mean_shift) {
  level_type *L = &us->s.level_h;
  if (!f) return HPGMG_USER_BAD_ARGUMENT;
  if (us->mask) return user_rhs_lifted(us, f, NULL, where, mean_shift);     /* Neumann walls: zero data on every face, the F-cycle keeps its hook */
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

/* boundary values (DESIGN.md §11): g_l and phi_l of every level, g and phi of apply_dirichlet -- 6 n_l^2 doubles each, allocated once */
static void user_bnd_alloc(hpgmg_user_solver *us) {
  const mg_type *G = &us->s.mg;
  int l;
  if (us->bnd_g) return;
  us->bnd_g = (double **)calloc((size_t)G->num_levels, sizeof(double *));
  us->bnd_phi = (double **)calloc((size_t)G->num_levels, sizeof(double *));
  if (us->mask) us->wall = (double **)calloc((size_t)G->num_levels, sizeof(double *));
  if (us->robin_mask) us->kappa = (double **)calloc((size_t)G->num_levels, sizeof(double *));
  for (l = 0; l < G->num_levels; l++) {
    const size_t n = (size_t)G->levels[l]->dim.i;
    us->bnd_g[l] = hpgmg_vector_alloc(6 * n * n);
    us->bnd_phi[l] = hpgmg_vector_alloc(6 * n * n);
    if (us->mask) us->wall[l] = l ? hpgmg_vector_alloc(6 * n * n) : us->wall0;
    if (us->robin_mask) us->kappa[l] = hpgmg_vector_alloc(6 * n * n);
  }
  us->app_g = hpgmg_vector_alloc((size_t)6 * us->n * us->n);
  us->app_phi = hpgmg_vector_alloc((size_t)6 * us->n * us->n);
}
static void user_bnd_take(hpgmg_user_solver *us, double *dst, const double *g, int where) {     /* the caller's g into plugin memory */
  const size_t len = (size_t)6 * us->n * us->n;
  if (where == HPGMG_WHERE_HOST) hpgmg_vector_upload(dst, g, len);
  else hpgmg_vector_copy(dst, g, len);
}

int hpgmg_user_set_rhs(hpgmg_user_solver *us, const double *f, int where, double *mean_shift) {
  us->march = 0;
  return user_rhs_plain(us, f, where, mean_shift);
}
int hpgmg_user_set_rhs_dirichlet(hpgmg_user_solver *us, const double *f, const double *g, int where, double *mean_shift) {
  us->march = 0;
  return user_rhs_lifted(us, f, g, where, mean_shift);
}

static int user_rhs_lifted(hpgmg_user_solver *us, const double *f, const double *g, int where, double *mean_shift) {
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
  const int st = user_pack_status(us->mask ? hpgmg_dense_pack_lifted_robin(L, VECTOR_F, f, where, us->bnd_g[0], s->b, us->mask, us->wall[0], USER_KAPPA(us, 0))
                                           : hpgmg_dense_pack_lifted(L, VECTOR_F, f, where, us->bnd_g[0], s->b));     /* F = f + T(g) */
  us->rhs_ok = (st == HPGMG_USER_OK);
  if (us->rhs_ok) {                  /* g_l and phi_l of every level, for the F-cycle's right-hand-side correction */
    for (l = 0; l < s->mg.num_levels; l++) {
      if (l > 0) hpgmg_boundary_restrict(s->mg.levels[l], us->bnd_g[l], s->mg.levels[l - 1], us->bnd_g[l - 1]);
      if (us->mask) hpgmg_boundary_flux_robin(s->mg.levels[l], us->bnd_phi[l], us->bnd_g[l], s->b, us->mask, us->wall[l], USER_KAPPA(us, l));
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
  if (us->mask) hpgmg_boundary_interp_robin(G->levels[l], e_id, G->levels[l + 1], us->bnd_g[l + 1], us->mask, USER_KAPPA(us, l + 1));
  else hpgmg_boundary_interp(G->levels[l], e_id, G->levels[l + 1], us->bnd_g[l + 1]);
}

int hpgmg_user_solve(hpgmg_user_solver *us, int method, double rtol, const double *u0, int where, hpgmg_user_info *info) {
  hpgmg_solver *s = &us->s;
  level_type *L = &s->level_h;
  if ((method != HPGMG_USER_FMG && method != HPGMG_USER_MG && method != HPGMG_USER_PCG && method != HPGMG_USER_FPCG) || !(rtol > 0.0)) return HPGMG_USER_BAD_ARGUMENT;
  if (!us->operator_ok || !us->rhs_ok) return HPGMG_USER_NOT_READY;
  if (!user_config_ok()) return HPGMG_USER_CONFLICT;
  USER_QUIET(us);
  us->march = 0;
  const int v0 = L->vcycles_from_this_level;
  double norm_of_F, r;
  if (method == HPGMG_USER_PCG || method == HPGMG_USER_FPCG) {    /* CG around the V-cycle, from u0 or from 0 (DESIGN.md §11.3, §11.4) */
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
  int st = user_pack_status(us->mask ? hpgmg_boundary_flux_robin(L, us->app_phi, us->app_g, s->b, us->mask, us->wall[0], USER_KAPPA(us, 0))
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

int hpgmg_user_flux(hpgmg_user_solver *us, const double *u, const double *g, double *flux_i, double *flux_j, double *flux_k, int where) {
  hpgmg_solver *s = &us->s;
  level_type *L = &s->level_h;
  if (!u || !flux_i || !flux_j || !flux_k || (where != HPGMG_WHERE_HOST && where != HPGMG_WHERE_PLUGIN)) return HPGMG_USER_BAD_ARGUMENT;
  if (g && us->bc != BC_DIRICHLET) return HPGMG_USER_UNSUPPORTED;
  if (!us->operator_ok) return HPGMG_USER_NOT_READY;
  if (!user_config_ok()) return HPGMG_USER_CONFLICT;
  USER_QUIET(us);
  int st = user_pack_status(hpgmg_dense_pack(L, us->x_id, u, where, HPGMG_DENSE_CELL, HPGMG_DENSE_CHECK_FINITE));
  if (st == HPGMG_USER_OK) {
    if (g) { user_bnd_alloc(us); user_bnd_take(us, us->app_g, g, where); }
    exchange_boundary(L, us->x_id, stencil_get_shape());      /* the neighbours across box faces and the periodic wrap; no ghost outside the domain is read */
    st = user_pack_status(hpgmg_dense_unpack_flux(L, us->x_id, g ? us->app_g : NULL, s->b, us->mask, us->mask ? us->wall[0] : NULL, USER_KAPPA(us, 0),
                                                  flux_i, flux_j, flux_k, where));
  }
  USER_LOUD();
  return st;
}

/* coefficient sensitivities (DESIGN.md §11.9): u into the operand vector, lam into VECTOR_R (apply's scratch: every solve sets it from f before
 * reading it), then one pass over both.  Nothing else is written: VECTOR_U, VECTOR_F, rhs_ok and a live march stay as they were. */
static int user_sensitivity(hpgmg_user_solver *us, const double *u, const double *lam, const double *kcell, int mean, const double *g, double *d_alpha,
                            double *d_beta_i, double *d_beta_j, double *d_beta_k, double *d_k, int where) {      /* kcell: into d_k; else into the d_beta */
  hpgmg_solver *s = &us->s;
  level_type *L = &s->level_h;
  if (!u || !lam || (where != HPGMG_WHERE_HOST && where != HPGMG_WHERE_PLUGIN)) return HPGMG_USER_BAD_ARGUMENT;
  if (kcell ? !d_k || (mean != HPGMG_MEAN_HARMONIC && mean != HPGMG_MEAN_ARITHMETIC) : !d_beta_i || !d_beta_j || !d_beta_k) return HPGMG_USER_BAD_ARGUMENT;
  if ((d_alpha != NULL) != (s->a != 0.0)) return HPGMG_USER_BAD_ARGUMENT;
  if (g && us->bc != BC_DIRICHLET) return HPGMG_USER_UNSUPPORTED;
  if (!us->operator_ok || !us->coef_given) return HPGMG_USER_NOT_READY;      /* no coefficient arrays (yet, or after a refused set_coefficients) */
  if (!user_config_ok()) return HPGMG_USER_CONFLICT;
  USER_QUIET(us);
  int st = user_pack_status(hpgmg_dense_pack(L, us->x_id, u, where, HPGMG_DENSE_CELL, HPGMG_DENSE_CHECK_FINITE));
  if (st == HPGMG_USER_OK) st = user_pack_status(hpgmg_dense_pack(L, VECTOR_R, lam, where, HPGMG_DENSE_CELL, HPGMG_DENSE_CHECK_FINITE));
  if (st == HPGMG_USER_OK) {
    const double *wall = us->mask ? us->wall[0] : NULL;
    if (g) { user_bnd_alloc(us); user_bnd_take(us, us->app_g, g, where); }
    exchange_boundary(L, us->x_id, stencil_get_shape());      /* the neighbours across box faces and the periodic wrap; no ghost outside the domain is read */
    exchange_boundary(L, VECTOR_R, stencil_get_shape());
    if (kcell) st = user_pack_status(hpgmg_dense_unpack_cell_sensitivity(L, us->x_id, VECTOR_R, kcell, mean, g ? us->app_g : NULL, s->a, s->b, us->mask, wall,
                                                                         USER_KAPPA(us, 0), d_alpha, d_k, where));
    else st = user_pack_status(hpgmg_dense_unpack_sensitivity(L, us->x_id, VECTOR_R, g ? us->app_g : NULL, s->a, s->b, us->mask, wall, USER_KAPPA(us, 0), d_alpha,
                                                              d_beta_i, d_beta_j, d_beta_k, where));
  }
  USER_LOUD();
  return st;
}
int hpgmg_user_sensitivity(hpgmg_user_solver *us, const double *u, const double *lam, const double *g, double *d_alpha, double *d_beta_i, double *d_beta_j,
                           double *d_beta_k, int where) {
  return user_sensitivity(us, u, lam, NULL, 0, g, d_alpha, d_beta_i, d_beta_j, d_beta_k, NULL, where);
}
/* the same with the chain rule through the face mean of a cell field (DESIGN.md §11.10): d_k in place of the three face arrays */
int hpgmg_user_cell_sensitivity(hpgmg_user_solver *us, const double *u, const double *lam, const double *kcell, int mean, const double *g, double *d_alpha,
                                double *d_k, int where) {
  if (!kcell) return HPGMG_USER_BAD_ARGUMENT;
  return user_sensitivity(us, u, lam, kcell, mean, g, d_alpha, NULL, NULL, NULL, d_k, where);
}


/* ---- implicit time stepping (DESIGN.md §11.8):  alpha du/dt = b div(beta grad u) + f  by the theta scheme.  With L(u; g) = A0 u - T(g) - a alpha u
 * (the operator without its a alpha term), the rate w = f - L(u; g) = alpha du/dt, a = 1 / (theta dt) and c = (1 - theta) / theta one step is the solve
 *   A0 u1 = f1 + T(g1) + a alpha u0 + c w0                                                                                      (1)
 * and, r being the residual of (1) the solve stopped at,
 *   w1 = r + a alpha (u1 - u0) - c w0                                                                                           (2)
 * exactly, whatever the tolerance.  The state u (VECTOR_U), u0 (uold_id) and w (w_id) stay on the finest level in the box layout between calls. */
static int user_theta_ok(double dt, double theta) { return isfinite(dt) && dt > 0.0 && theta >= 0.5 && theta <= 1.0 && isfinite(1.0 / (theta * dt)); }
static int user_march_rhs(hpgmg_user_solver *us, const double *f, const double *g, int where) {      /* VECTOR_F = f + T(g), under set_rhs's rules for g */
  return (g || us->mask) ? user_rhs_lifted(us, f, g, where, NULL) : user_rhs_plain(us, f, where, NULL);
}

int hpgmg_user_set_shift(hpgmg_user_solver *us, double a) {
  if (!us || us->s.a == 0.0 || !isfinite(a) || !(a > 0.0)) return HPGMG_USER_BAD_ARGUMENT;      /* a Poisson solver stays one: the helmholtz flag is process-wide */
  if (!us->operator_ok) return HPGMG_USER_NOT_READY;
  if (!user_config_ok()) return HPGMG_USER_CONFLICT;
  USER_QUIET(us);
  us->s.a = a;
  user_rebuild(us);                      /* no pack: the coefficient vectors, wall[0] and kappa[0] are the ones set_coefficients left; F and every phi_l do not depend on a */
  USER_LOUD();
  return HPGMG_USER_OK;
}

int hpgmg_user_start(hpgmg_user_solver *us, const double *u, const double *f, const double *g, int where, double dt, double theta) {
  if (!us || !u || !f || (where != HPGMG_WHERE_HOST && where != HPGMG_WHERE_PLUGIN)) return HPGMG_USER_BAD_ARGUMENT;
  hpgmg_solver *s = &us->s;
  level_type *L = &s->level_h;
  if (s->a == 0.0 || !user_theta_ok(dt, theta)) return HPGMG_USER_BAD_ARGUMENT;
  if (g && us->bc != BC_DIRICHLET) return HPGMG_USER_UNSUPPORTED;
  if (!us->operator_ok) return HPGMG_USER_NOT_READY;
  if (!user_config_ok()) return HPGMG_USER_CONFLICT;
  if (L->must_subtract_mean == 1) return HPGMG_USER_UNSUPPORTED;      /* alpha is 0 everywhere: there is no du/dt term to march */
  us->march = 0;
  USER_QUIET(us);
  if (!us->uold_id) {                    /* the first march: two more vectors on the finest level (a solver that never starts keeps its count) */
    us->uold_id = L->numVectors; us->w_id = L->numVectors + 1;
    create_vectors(L, L->numVectors + 2);
  }
  const double a = 1.0 / (theta * dt), c = (1.0 - theta) / theta;
  int st = user_pack_status(hpgmg_dense_pack(L, VECTOR_U, u, where, HPGMG_DENSE_CELL, HPGMG_DENSE_CHECK_FINITE));
  if (st == HPGMG_USER_OK) st = user_march_rhs(us, f, g, where);
  if (st == HPGMG_USER_OK && a != s->a) st = hpgmg_user_set_shift(us, a);      /* after the packs: a refused array leaves the operator as it was */
  if (st == HPGMG_USER_OK) {           /* (2) with u0 = 0, w0 = 0: w = r + a alpha u = f - L(u; g) */
    double rate;
    residual(L, VECTOR_TEMP, VECTOR_U, VECTOR_F, s->a, s->b);
    zero_vector(L, us->uold_id);
    zero_vector(L, us->w_id);
    hpgmg_step_rate(L, us->w_id, VECTOR_TEMP, VECTOR_U, us->uold_id, s->a, c, &rate);
    us->dt = dt; us->theta = theta;
    us->march = 1;
  }
  USER_LOUD();
  return st;
}

int hpgmg_user_step(hpgmg_user_solver *us, const double *f, const double *g, int where, double dt, double theta, double rtol, hpgmg_user_info *info,
                    double *rate) {
  if (!us || !f || !(rtol > 0.0) || (where != HPGMG_WHERE_HOST && where != HPGMG_WHERE_PLUGIN)) return HPGMG_USER_BAD_ARGUMENT;
  hpgmg_solver *s = &us->s;
  level_type *L = &s->level_h;
  if (us->march != 1 || !us->operator_ok) return HPGMG_USER_NOT_READY;      /* no march, or a wave march */
  if (!(dt > 0.0)) dt = us->dt;          /* <= 0: as before */
  if (!(theta > 0.0)) theta = us->theta;
  if (!user_theta_ok(dt, theta)) return HPGMG_USER_BAD_ARGUMENT;
  if (g && us->bc != BC_DIRICHLET) return HPGMG_USER_UNSUPPORTED;
  if (!user_config_ok()) return HPGMG_USER_CONFLICT;
  USER_QUIET(us);
  const int st = user_march_rhs(us, f, g, where);      /* F = f + T(g), g_l and phi_l: a refusal (f or g not finite) ends here, u, w and the march intact */
  if (st != HPGMG_USER_OK) { USER_LOUD(); return st; }
  const double a = 1.0 / (theta * dt), c = (1.0 - theta) / theta;
  if (a != s->a) {                       /* w does not depend on a: it stays valid across the change */
    const int e = hpgmg_user_set_shift(us, a);
    if (e != HPGMG_USER_OK) { USER_LOUD(); return e; }
  }
  us->dt = dt; us->theta = theta;
  const int v0 = L->vcycles_from_this_level;
  double w_max;
  hpgmg_step_rhs(L, VECTOR_F, VECTOR_U, us->uold_id, us->w_id, s->a, c);      /* (1)'s right-hand side; u_old = u */
  us->rhs_ok = 0;                        /* VECTOR_F is no longer the caller's f + T(g): a solve needs its own set_rhs */
  /* the warm start of hpgmg_user_solve from the state the library holds: u = u_old + e with A e = F - A u_old */
  residual(L, us->x_id, VECTOR_U, VECTOR_F, s->a, s->b);
  const double norm_of_F = norm(L, VECTOR_F), norm_of_r0 = norm(L, us->x_id);
  if (norm_of_r0 > 0.0) {
    MGSolve(&s->mg, 0, VECTOR_U, us->x_id, s->a, s->b, rtol * norm_of_F / norm_of_r0);
    add_vectors(L, VECTOR_U, 1.0, VECTOR_U, 1.0, us->uold_id);
  }
  residual(L, VECTOR_TEMP, VECTOR_U, VECTOR_F, s->a, s->b);
  const double r = norm(L, VECTOR_TEMP);
  hpgmg_step_rate(L, us->w_id, VECTOR_TEMP, VECTOR_U, us->uold_id, s->a, c, &w_max);      /* (2) */
  USER_LOUD();
  if (info) {
    info->norm_of_residual = r; info->norm_of_f = norm_of_F; info->mean_shift = 0.0;
    info->vcycles = L->vcycles_from_this_level - v0;
    info->converged = (r == 0.0) || (r < rtol * norm_of_F);
  }
  if (rate) *rate = w_max;
  return HPGMG_USER_OK;
}

int hpgmg_user_get_rate(hpgmg_user_solver *us, double *out, int where) {
  if (!us || !out) return HPGMG_USER_BAD_ARGUMENT;
  if (us->march != 1) return HPGMG_USER_NOT_READY;
  USER_QUIET(us);
  const int st = hpgmg_dense_unpack(&us->s.level_h, us->w_id, out, where);
  USER_LOUD();
  return st < 0 ? HPGMG_USER_BAD_ARGUMENT : HPGMG_USER_OK;
}
