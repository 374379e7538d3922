/*
 * plugin_dense.c -- hpgmg_dense_pack / hpgmg_dense_unpack / hpgmg_dense_unpack_flux / hpgmg_dense_unpack_sensitivity of the operator plugin
 * (include/hpgmg_operators.h): one launch of kernels/dense_io.hip per array (the three flux arrays: one of kernels/dense_flux.hip; the four
 * sensitivity arrays: one of kernels/dense_sensitivity.hip; a cell-centred conductivity: kernels/dense_cells.hip).  A device array is read / written in place; a host array is copied once into the level's staging buffer
 * (allocated on first use, freed with the level) and packed from there, or unpacked into it and copied out once.  They replace the weak
 * host defaults of host/hooks_host.inc, which go box by box through hpgmg_vector_upload / download.  The boundary-value hooks below likewise
 * (their arithmetic: include/hpgmg_boundary_math.h, shared with the kernels and the host defaults).
 */
#include "plugin_internal.h"
#include "hpgmg_boundary_math.h"

static double *dense_stage(backend_t *B, size_t n) {
  if (B->dense_stage_len < n) {
    if (B->dense_stage) hpgmg_hip_free(B->dense_stage);
    B->dense_stage = (double *)hpgmg_hip_malloc(n * sizeof(double));
    B->dense_stage_len = B->dense_stage ? n : 0;
    if (!B->dense_stage) { fprintf(stderr, "hpgmg: dense arrays: no device memory for a %zu-double staging buffer\n", n); abort(); }
  }
  return B->dense_stage;
}
/* what every pack checks first, then the caller's len doubles at src where the kernels can read them: in place for a device array, else
 * copied once into the staging buffer.  NULL: the call is refused */
static const double *dense_source(level_type *L, int id, const double *src, int where, size_t len) {
  if (L->num_ranks != 1 || id < 0 || id >= L->numVectors || !src) return NULL;
  if (where == HPGMG_WHERE_PLUGIN) return src;
  if (where != HPGMG_WHERE_HOST) return NULL;
  double *stage = dense_stage(hp_backend_of(L), len);
  HIP_OK(hpgmg_hip_memcpy_h2d(stage, src, len * sizeof(double)));
  return stage;
}
static void dense_extents(const level_type *L, int layout, size_t n[3]) {      /* of a dense array of that layout, i, j, k */
  const int high = L->boundary_condition.type == BC_DIRICHLET;
  n[0] = (size_t)dense_extent(L->dim.i, high && layout == HPGMG_DENSE_FACE_I);
  n[1] = (size_t)dense_extent(L->dim.j, high && layout == HPGMG_DENSE_FACE_J);
  n[2] = (size_t)dense_extent(L->dim.k, high && layout == HPGMG_DENSE_FACE_K);
}

int hpgmg_dense_pack(level_type *L, int id, const double *src, int where, int layout, int check) {
  size_t n[3];
  int status = 0;
  if (layout < HPGMG_DENSE_CELL || layout > HPGMG_DENSE_FACE_K) return -1;
  dense_extents(L, layout, n);
  if (!(src = dense_source(L, id, src, where, n[0] * n[1] * n[2]))) return -1;
  hp_coef_written(L, id);
  HIP_OK(hpgmg_hip_dense_pack(&hp_backend_of(L)->dev, id, src, (int)n[0], (int)n[1], (int)n[2], check, &status));
  return status;
}

int hpgmg_dense_unpack(level_type *L, int id, double *dst, int where) {
  if (L->num_ranks != 1 || id < 0 || id >= L->numVectors || !dst) return -1;
  if (where != HPGMG_WHERE_HOST && where != HPGMG_WHERE_PLUGIN) return -1;
  backend_t *B = hp_backend_of(L);
  const size_t n = (size_t)L->dim.i * L->dim.j * L->dim.k;
  if (where == HPGMG_WHERE_PLUGIN) { HIP_OK(hpgmg_hip_dense_unpack(&B->dev, id, dst)); return 0; }
  double *stage = dense_stage(B, n);
  HIP_OK(hpgmg_hip_dense_unpack(&B->dev, id, stage));
  HIP_OK(hpgmg_hip_memcpy_d2h(dst, stage, n * sizeof(double)));
  return 0;
}

/* face fluxes of vector x_id: one launch of kernels/dense_flux.hip for the three arrays, written in place when they are device
 * arrays, else into the staging buffer (sized for the three) and copied out, one copy each */
int hpgmg_dense_unpack_flux(level_type *L, int x_id, const double *g, double b, int mask, const double *wall, const double *kappa,
                            double *flux_i, double *flux_j, double *flux_k, int where) {
  int status = 0;
  if (L->num_ranks != 1 || x_id < 0 || x_id >= L->numVectors || !flux_i || !flux_j || !flux_k) return -1;
  if (where != HPGMG_WHERE_HOST && where != HPGMG_WHERE_PLUGIN) return -1;
  if (mask < 0 || mask > 63 || (mask && !wall) || L->dim.i != L->dim.j || L->dim.i != L->dim.k || L->box_ghosts < 1) return -1;
  if (L->boundary_condition.type != BC_DIRICHLET && (g || mask)) return -1;
  backend_t *B = hp_backend_of(L);
  const double wq = bnd_weight_neumann(b, L->h);
  if (where == HPGMG_WHERE_PLUGIN) {
    HIP_OK(hpgmg_hip_dense_unpack_flux(&B->dev, x_id, g, b, wq, L->h, mask, wall, mask ? kappa : NULL, flux_i, flux_j, flux_k, &status));
    return status;
  }
  size_t n[3];
  dense_extents(L, HPGMG_DENSE_FACE_I, n);
  const size_t len = n[0] * n[1] * n[2];          /* of each of the three: the level is a cube */
  double *stage = dense_stage(B, 3 * len);
  HIP_OK(hpgmg_hip_dense_unpack_flux(&B->dev, x_id, g, b, wq, L->h, mask, wall, mask ? kappa : NULL, stage, stage + len, stage + 2 * len, &status));
  HIP_OK(hpgmg_hip_memcpy_d2h(flux_i, stage, len * sizeof(double)));
  HIP_OK(hpgmg_hip_memcpy_d2h(flux_j, stage + len, len * sizeof(double)));
  HIP_OK(hpgmg_hip_memcpy_d2h(flux_k, stage + 2 * len, len * sizeof(double)));
  return status;
}

/* coefficient sensitivities of vectors u_id and lam_id: one launch of kernels/dense_sensitivity.hip for the four arrays, written in
 * place when they are device arrays, else into the staging buffer (sized for the four) and copied out, one copy each */
int hpgmg_dense_unpack_sensitivity(level_type *L, int u_id, int lam_id, const double *g, double a, double b, int mask, const double *wall,
                                   const double *kappa, double *d_alpha, double *d_beta_i, double *d_beta_j, double *d_beta_k, int where) {
  int status = 0;
  if (L->num_ranks != 1 || u_id < 0 || u_id >= L->numVectors || lam_id < 0 || lam_id >= L->numVectors || !d_beta_i || !d_beta_j || !d_beta_k) return -1;
  if (where != HPGMG_WHERE_HOST && where != HPGMG_WHERE_PLUGIN) return -1;
  if (mask < 0 || mask > 63 || (mask && !wall) || L->dim.i != L->dim.j || L->dim.i != L->dim.k || L->box_ghosts < 1) return -1;
  if (L->boundary_condition.type != BC_DIRICHLET && (g || mask)) return -1;
  backend_t *B = hp_backend_of(L);
  const double w2 = bnd_sens_weight(b, L->h), w = bnd_weight(b, L->h), wn = bnd_weight_neumann(b, L->h);
  if (where == HPGMG_WHERE_PLUGIN) {
    HIP_OK(hpgmg_hip_dense_unpack_sensitivity(&B->dev, u_id, lam_id, g, a, w2, w, wn, L->h, mask, mask ? kappa : NULL, d_alpha, d_beta_i, d_beta_j,
                                              d_beta_k, &status));
    return status;
  }
  size_t n[3];
  dense_extents(L, HPGMG_DENSE_FACE_I, n);
  const size_t len = n[0] * n[1] * n[2], cells = (size_t)L->dim.i * L->dim.j * L->dim.k;      /* of each face array (the level is a cube), of d_alpha */
  double *stage = dense_stage(B, 3 * len + cells);
  HIP_OK(hpgmg_hip_dense_unpack_sensitivity(&B->dev, u_id, lam_id, g, a, w2, w, wn, L->h, mask, mask ? kappa : NULL, d_alpha ? stage + 3 * len : NULL,
                                            stage, stage + len, stage + 2 * len, &status));
  HIP_OK(hpgmg_hip_memcpy_d2h(d_beta_i, stage, len * sizeof(double)));
  HIP_OK(hpgmg_hip_memcpy_d2h(d_beta_j, stage + len, len * sizeof(double)));
  HIP_OK(hpgmg_hip_memcpy_d2h(d_beta_k, stage + 2 * len, len * sizeof(double)));
  if (d_alpha) HIP_OK(hpgmg_hip_memcpy_d2h(d_alpha, stage + 3 * len, cells * sizeof(double)));
  return status;
}

/* cell-centred conductivities: one launch of kernels/dense_cells.hip each.  A host kcell is staged like any pack's array; the
 * cell sensitivities' host outputs follow it in the staging buffer (3 cells in all: within the 3 len + cells the sensitivities above size it to) */
int hpgmg_dense_pack_cell_mean(level_type *L, const double *kcell, int where, int mean, int mask, double *wall) {
  int status = 0;
  if (L->dim.i != L->dim.j || L->dim.i != L->dim.k || (mean != HPGMG_MEAN_HARMONIC && mean != HPGMG_MEAN_ARITHMETIC)) return -1;
  if (mask < 0 || mask > 63 || (mask && (!wall || L->boundary_condition.type != BC_DIRICHLET))) return -1;
  if (!(kcell = dense_source(L, VECTOR_BETA_I, kcell, where, (size_t)L->dim.i * L->dim.j * L->dim.k))) return -1;
  hp_coef_written(L, VECTOR_BETA_I);      /* and J, K: one record covers the coefficient vectors */
  HIP_OK(hpgmg_hip_dense_pack_cell_mean(&hp_backend_of(L)->dev, VECTOR_BETA_I, VECTOR_BETA_J, VECTOR_BETA_K, kcell, mean, mask, mask ? wall : NULL, &status));
  return status;
}

int hpgmg_dense_unpack_cell_sensitivity(level_type *L, int u_id, int lam_id, const double *kcell, int mean, const double *g, double a, double b, int mask,
                                        const double *wall, const double *kappa, double *d_alpha, double *d_k, int where) {
  int status = 0;
  if (L->num_ranks != 1 || u_id < 0 || u_id >= L->numVectors || lam_id < 0 || lam_id >= L->numVectors || !kcell || !d_k) return -1;
  if (where != HPGMG_WHERE_HOST && where != HPGMG_WHERE_PLUGIN) return -1;
  if (mean != HPGMG_MEAN_HARMONIC && mean != HPGMG_MEAN_ARITHMETIC) return -1;
  if (mask < 0 || mask > 63 || (mask && !wall) || L->dim.i != L->dim.j || L->dim.i != L->dim.k || L->box_ghosts < 1) return -1;
  if (L->boundary_condition.type != BC_DIRICHLET && (g || mask)) return -1;
  backend_t *B = hp_backend_of(L);
  const double w2 = bnd_sens_weight(b, L->h), w = bnd_weight(b, L->h), wn = bnd_weight_neumann(b, L->h);
  if (where == HPGMG_WHERE_PLUGIN) {
    HIP_OK(hpgmg_hip_dense_unpack_cell_sensitivity(&B->dev, u_id, lam_id, kcell, mean, g, a, w2, w, wn, L->h, mask, mask ? kappa : NULL, d_alpha, d_k, &status));
    return status;
  }
  const size_t cells = (size_t)L->dim.i * L->dim.j * L->dim.k;
  double *stage = dense_stage(B, 3 * cells);
  HIP_OK(hpgmg_hip_memcpy_h2d(stage, kcell, cells * sizeof(double)));
  HIP_OK(hpgmg_hip_dense_unpack_cell_sensitivity(&B->dev, u_id, lam_id, stage, mean, g, a, w2, w, wn, L->h, mask, mask ? kappa : NULL,
                                                 d_alpha ? stage + 2 * cells : NULL, stage + cells, &status));
  HIP_OK(hpgmg_hip_memcpy_d2h(d_k, stage + cells, cells * sizeof(double)));
  if (d_alpha) HIP_OK(hpgmg_hip_memcpy_d2h(d_alpha, stage + 2 * cells, cells * sizeof(double)));
  return status;
}

/* boundary values (include/hpgmg_operators.h): one launch of kernels/dense_boundary.hip each.  g, phi, wall are device arrays
 * (hpgmg_vector_alloc); f is staged as hpgmg_dense_pack stages it.  The plain forms are the per-face forms without a Neumann wall. */
int hpgmg_dense_pack_walls(level_type *L, int id, const double *src, int where, int layout, int check, int mask, double *wall) {
  size_t n[3];
  int status = 0;
  if (layout < HPGMG_DENSE_FACE_I || layout > HPGMG_DENSE_FACE_K || !wall) return -1;
  if (mask < 0 || mask > 63 || L->boundary_condition.type != BC_DIRICHLET || L->dim.i != L->dim.j || L->dim.i != L->dim.k) return -1;
  dense_extents(L, layout, n);
  if (!(src = dense_source(L, id, src, where, n[0] * n[1] * n[2]))) return -1;
  hp_coef_written(L, id);
  HIP_OK(hpgmg_hip_dense_pack_walls(&hp_backend_of(L)->dev, id, src, layout - HPGMG_DENSE_FACE_I, check, mask, wall, &status));
  return status;
}

int hpgmg_dense_pack_lifted_robin(level_type *L, int id, const double *f, int where, const double *g, double b, int mask, const double *wall, const double *kappa) {
  int status = 0;
  if (!g || L->boundary_condition.type != BC_DIRICHLET || mask < 0 || mask > 63 || (mask && !wall)) return -1;
  if (!(f = dense_source(L, id, f, where, (size_t)L->dim.i * L->dim.j * L->dim.k))) return -1;
  hp_coef_written(L, id);
  HIP_OK(hpgmg_hip_dense_pack_lifted_robin(&hp_backend_of(L)->dev, id, f, g, bnd_weight(b, L->h), mask, wall, bnd_weight_neumann(b, L->h),
                                           mask ? kappa : NULL, L->h, &status));
  return status;
}
int hpgmg_dense_pack_lifted_faces(level_type *L, int id, const double *f, int where, const double *g, double b, int mask, const double *wall) {
  return hpgmg_dense_pack_lifted_robin(L, id, f, where, g, b, mask, wall, NULL);
}
int hpgmg_dense_pack_lifted(level_type *L, int id, const double *f, int where, const double *g, double b) {
  return hpgmg_dense_pack_lifted_faces(L, id, f, where, g, b, 0, NULL);
}

int hpgmg_boundary_flux_robin(level_type *L, double *phi, const double *g, double b, int mask, const double *wall, const double *kappa) {
  int status = 0;
  if (mask < 0 || mask > 63 || (mask && !wall)) return -1;
  HIP_OK(hpgmg_hip_boundary_flux_robin(&hp_backend_of(L)->dev, phi, g, bnd_weight(b, L->h), mask, wall, bnd_weight_neumann(b, L->h), mask ? kappa : NULL, L->h,
                                       &status));
  return status;
}
int hpgmg_boundary_flux_faces(level_type *L, double *phi, const double *g, double b, int mask, const double *wall) {
  return hpgmg_boundary_flux_robin(L, phi, g, b, mask, wall, NULL);
}
int hpgmg_boundary_flux(level_type *L, double *phi, const double *g, double b) { return hpgmg_boundary_flux_faces(L, phi, g, b, 0, NULL); }

void hpgmg_boundary_restrict(level_type *Lc, double *g_c, level_type *Lf, const double *g_f) {
  (void)Lf;
  HIP_OK(hpgmg_hip_boundary_restrict(g_c, g_f, Lc->dim.i));
}

void hpgmg_boundary_lift(level_type *L, int id, const double *phi, const double *phi_fine, double sign) {
  hp_coef_written(L, id);
  HIP_OK(hpgmg_hip_boundary_lift(&hp_backend_of(L)->dev, id, phi, phi_fine, sign));
}

void hpgmg_boundary_interp(level_type *Lf, int id, level_type *Lc, const double *g_c) {
  HIP_OK(hpgmg_hip_boundary_interp(&hp_backend_of(Lf)->dev, id, g_c, Lc->dim.i));
}

void hpgmg_boundary_interp_robin(level_type *Lf, int id, level_type *Lc, const double *g_c, int mask, const double *kappa_c) {
  int nb = Lc->dim.i / Lc->box_dim, bx;          /* the kernel's box formula holds when the coarse boxes are in i-fastest order */
  if (Lc->num_my_boxes != nb * nb * nb) nb = 0;
  for (bx = 0; nb && bx < Lc->num_my_boxes; bx++) {
    const box_type *X = &Lc->my_boxes[bx];
    if (X->low.i != (bx % nb) * Lc->box_dim || X->low.j != ((bx / nb) % nb) * Lc->box_dim || X->low.k != (bx / (nb * nb)) * Lc->box_dim) nb = 0;
  }
  HIP_OK(hpgmg_hip_boundary_interp_robin(&hp_backend_of(Lf)->dev, id, &hp_backend_of(Lc)->dev, nb, g_c, Lc->h, mask, mask ? kappa_c : NULL));
}
void hpgmg_boundary_interp_faces(level_type *Lf, int id, level_type *Lc, const double *g_c, int mask) {
  hpgmg_boundary_interp_robin(Lf, id, Lc, g_c, mask, NULL);
}

/* Robin walls: a host array of kappa is staged as hpgmg_dense_pack stages its array */
int hpgmg_boundary_check_kappa(level_type *L, const double *kappa, int where, int robin_mask, int *any_positive) {
  int status = 0;
  if (any_positive) *any_positive = 0;
  if (robin_mask < 0 || robin_mask > 63 || L->dim.i != L->dim.j || L->dim.i != L->dim.k) return -1;
  if (!(kappa = dense_source(L, 0, kappa, where, (size_t)6 * L->dim.i * L->dim.i))) return -1;
  HIP_OK(hpgmg_hip_boundary_check_kappa(kappa, L->dim.i, robin_mask, &status));
  if (any_positive) *any_positive = (status & BND_KAPPA_POSITIVE) != 0;
  return status & (HPGMG_DENSE_NOT_FINITE | HPGMG_DENSE_OUT_OF_RANGE);
}
void hpgmg_boundary_store_walls(level_type *L, const double *wall, const double *kappa, int mask) {
  if (!mask || !wall) return;
  hp_dinv_record_clear(L);                             /* the wall betas change: VECTOR_DINV is stale until the next rebuild_operator */
  HIP_OK(hpgmg_hip_boundary_store_walls(&hp_backend_of(L)->dev, wall, kappa, L->h, mask));
}
