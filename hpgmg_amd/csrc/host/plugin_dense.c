/*
 * plugin_dense.c -- hpgmg_dense_pack / hpgmg_dense_unpack of the operator plugin (include/hpgmg_operators.h): one launch of
 * kernels/dense_io.hip per array.  A device array is read / written in place; a host array is copied once into the level's staging buffer
 * (allocated on first use, freed with the level) and packed from there, or unpacked into it and copied out once.  They replace the weak
 * host defaults of host/driver.c, which go box by box through hpgmg_vector_upload / download.  The boundary-value hooks below likewise.
 */
#include "plugin_internal.h"

static size_t dense_extent(const level_type *L, int layout, int axis) {     /* axis 0 = i, 1 = j, 2 = k */
  const int n = axis == 0 ? L->dim.i : axis == 1 ? L->dim.j : L->dim.k;
  return (size_t)n + (layout == HPGMG_DENSE_FACE_I + axis && L->boundary_condition.type == BC_DIRICHLET);
}

static double *dense_stage(backend_t *B, size_t n) {
  if (B->dense_stage_len < n) {
    if (B->dense_stage) hpgmg_hip_free(B->dense_stage);
    B->dense_stage = (double *)hpgmg_hip_malloc(n * sizeof(double));
    B->dense_stage_len = B->dense_stage ? n : 0;
    if (!B->dense_stage) { fprintf(stderr, "hpgmg: dense arrays: no device memory for a %zu-double staging buffer\n", n); abort(); }
  }
  return B->dense_stage;
}

int hpgmg_dense_pack(level_type *L, int id, const double *src, int where, int layout, int check) {
  if (L->num_ranks != 1 || id < 0 || id >= L->numVectors || layout < HPGMG_DENSE_CELL || layout > HPGMG_DENSE_FACE_K || !src) return -1;
  if (where != HPGMG_WHERE_HOST && where != HPGMG_WHERE_PLUGIN) return -1;
  backend_t *B = hp_backend_of(L);
  const size_t ni = dense_extent(L, layout, 0), nj = dense_extent(L, layout, 1), nk = dense_extent(L, layout, 2);
  const double *d_src = src;
  int status = 0;
  if (where == HPGMG_WHERE_HOST) {
    double *stage = dense_stage(B, ni * nj * nk);
    HIP_OK(hpgmg_hip_memcpy_h2d(stage, src, ni * nj * nk * sizeof(double)));
    d_src = stage;
  }
  HIP_OK(hpgmg_hip_dense_pack(&B->dev, id, d_src, (int)ni, (int)nj, (int)nk, check, &status));
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

/* boundary values (include/hpgmg_operators.h): one launch of kernels/dense_boundary.hip each.  g, phi are device arrays (hpgmg_vector_alloc);
 * f is staged as hpgmg_dense_pack stages it. */
static double bnd_weight(const level_type *L, double b) { return (2.0 * b) * (1.0 / (L->h * L->h)); }

int hpgmg_dense_pack_lifted(level_type *L, int id, const double *f, int where, const double *g, double b) {
  if (L->num_ranks != 1 || id < 0 || id >= L->numVectors || !f || !g || L->boundary_condition.type != BC_DIRICHLET) return -1;
  if (where != HPGMG_WHERE_HOST && where != HPGMG_WHERE_PLUGIN) return -1;
  backend_t *B = hp_backend_of(L);
  const size_t n = (size_t)L->dim.i * L->dim.j * L->dim.k;
  const double *d_src = f;
  int status = 0;
  if (where == HPGMG_WHERE_HOST) {
    double *stage = dense_stage(B, n);
    HIP_OK(hpgmg_hip_memcpy_h2d(stage, f, n * sizeof(double)));
    d_src = stage;
  }
  HIP_OK(hpgmg_hip_dense_pack_lifted(&B->dev, id, d_src, g, bnd_weight(L, b), &status));
  return status;
}

int hpgmg_boundary_flux(level_type *L, double *phi, const double *g, double b) {
  int status = 0;
  HIP_OK(hpgmg_hip_boundary_flux(&hp_backend_of(L)->dev, phi, g, bnd_weight(L, b), &status));
  return status;
}

void hpgmg_boundary_restrict(level_type *Lc, double *g_c, level_type *Lf, const double *g_f) {
  (void)Lf;
  HIP_OK(hpgmg_hip_boundary_restrict(g_c, g_f, Lc->dim.i));
}

void hpgmg_boundary_lift(level_type *L, int id, const double *phi, const double *phi_fine, double sign) {
  HIP_OK(hpgmg_hip_boundary_lift(&hp_backend_of(L)->dev, id, phi, phi_fine, sign));
}

void hpgmg_boundary_interp(level_type *Lf, int id, level_type *Lc, const double *g_c) {
  HIP_OK(hpgmg_hip_boundary_interp(&hp_backend_of(Lf)->dev, id, g_c, Lc->dim.i));
}

/* Neumann walls (include/hpgmg_operators.h): the same launches with per-face kinds */
static double bnd_weight_neumann(const level_type *L, double b) { return b * (1.0 / L->h); }

int hpgmg_dense_pack_walls(level_type *L, int id, const double *src, int where, int layout, int check, int mask, double *wall) {
  if (L->num_ranks != 1 || id < 0 || id >= L->numVectors || layout < HPGMG_DENSE_FACE_I || layout > HPGMG_DENSE_FACE_K || !src || !wall) return -1;
  if (where != HPGMG_WHERE_HOST && where != HPGMG_WHERE_PLUGIN) return -1;
  if (mask < 0 || mask > 63 || L->boundary_condition.type != BC_DIRICHLET || L->dim.i != L->dim.j || L->dim.i != L->dim.k) return -1;
  backend_t *B = hp_backend_of(L);
  const size_t ni = dense_extent(L, layout, 0), nj = dense_extent(L, layout, 1), nk = dense_extent(L, layout, 2);
  const double *d_src = src;
  int status = 0;
  if (where == HPGMG_WHERE_HOST) {
    double *stage = dense_stage(B, ni * nj * nk);
    HIP_OK(hpgmg_hip_memcpy_h2d(stage, src, ni * nj * nk * sizeof(double)));
    d_src = stage;
  }
  HIP_OK(hpgmg_hip_dense_pack_walls(&B->dev, id, d_src, layout - HPGMG_DENSE_FACE_I, check, mask, wall, &status));
  return status;
}

int hpgmg_dense_pack_lifted_faces(level_type *L, int id, const double *f, int where, const double *g, double b, int mask, const double *wall) {
  if (L->num_ranks != 1 || id < 0 || id >= L->numVectors || !f || !g || L->boundary_condition.type != BC_DIRICHLET) return -1;
  if (where != HPGMG_WHERE_HOST && where != HPGMG_WHERE_PLUGIN) return -1;
  if (mask < 0 || mask > 63 || (mask && !wall)) return -1;
  backend_t *B = hp_backend_of(L);
  const size_t n = (size_t)L->dim.i * L->dim.j * L->dim.k;
  const double *d_src = f;
  int status = 0;
  if (where == HPGMG_WHERE_HOST) {
    double *stage = dense_stage(B, n);
    HIP_OK(hpgmg_hip_memcpy_h2d(stage, f, n * sizeof(double)));
    d_src = stage;
  }
  HIP_OK(hpgmg_hip_dense_pack_lifted_faces(&B->dev, id, d_src, g, bnd_weight(L, b), mask, wall, bnd_weight_neumann(L, b), &status));
  return status;
}

int hpgmg_boundary_flux_faces(level_type *L, double *phi, const double *g, double b, int mask, const double *wall) {
  int status = 0;
  if (mask < 0 || mask > 63 || (mask && !wall)) return -1;
  HIP_OK(hpgmg_hip_boundary_flux_faces(&hp_backend_of(L)->dev, phi, g, bnd_weight(L, b), mask, wall, bnd_weight_neumann(L, b), &status));
  return status;
}

void hpgmg_boundary_interp_faces(level_type *Lf, int id, level_type *Lc, const double *g_c, int mask) {
  int nb = Lc->dim.i / Lc->box_dim, bx;          /* the kernel's box formula holds when the coarse boxes are in i-fastest order */
  if (Lc->num_my_boxes != nb * nb * nb) nb = 0;
  for (bx = 0; nb && bx < Lc->num_my_boxes; bx++) {
    const box_type *X = &Lc->my_boxes[bx];
    if (X->low.i != (bx % nb) * Lc->box_dim || X->low.j != ((bx / nb) % nb) * Lc->box_dim || X->low.k != (bx / (nb * nb)) * Lc->box_dim) nb = 0;
  }
  HIP_OK(hpgmg_hip_boundary_interp_faces(&hp_backend_of(Lf)->dev, id, &hp_backend_of(Lc)->dev, nb, g_c, Lc->h, mask));
}
