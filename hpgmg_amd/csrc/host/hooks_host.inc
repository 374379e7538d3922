/*
 * hooks_host.inc -- the portable host forms of the dense-array, boundary-value, time-march and CG hooks (include/hpgmg_operators.h hpgmg_dense_*,
 * hpgmg_boundary_*, hpgmg_step_*, hpgmg_pcg_*, hpgmg_block_*, hpgmg_wave_*): box by box through the plugin's hpgmg_vector_upload / download.  They are weak, so that a plugin with kernels
 * for them (the HIP plugin: host/plugin_dense.c, host/plugin_pcg.c; its kernels: kernels/dense_io.hip, dense_boundary.hip, dense_flux.hip, dense_cells.hip, pcg.hip) replaces them while one without (the CPU oracle, whose memory is host memory
 * for either `where`) gets these.  The boundary arithmetic itself is include/hpgmg_boundary_math.h, shared with those kernels.
 * A part of host/driver.c's translation unit, included there.
 */
#include <stdlib.h>
#include <string.h>
#include <math.h>
#include "hpgmg_fv.h"
#include "hpgmg_boundary_math.h"
#include "hpgmg_step_math.h"
#include "hpgmg_wave_math.h"

/* ------------------------------------------------------------------ dense arrays <-> boxes (include/hpgmg_operators.h) */
/* mask, wall: hpgmg_dense_pack_walls (0, NULL: hpgmg_dense_pack) */
static int dense_pack_host(level_type *L, int id, const double *src, int where, int layout, int check, int mask, double *wall) {
  if (L->num_ranks != 1 || id < 0 || id >= L->numVectors || layout < HPGMG_DENSE_CELL || layout > HPGMG_DENSE_FACE_K || !src) return -1;
  if (where != HPGMG_WHERE_HOST && where != HPGMG_WHERE_PLUGIN) return -1;
  const int axis = layout - HPGMG_DENSE_FACE_I, n = L->dim.i;
  const int lo = mask ? (mask >> (2 * axis)) & 1 : 0, hi = mask ? (mask >> (2 * axis + 1)) & 1 : 0;
  double *wh = NULL;
  if (lo || hi) { wh = (double *)malloc((size_t)6 * n * n * sizeof(double)); hpgmg_vector_download(wh, wall, (size_t)6 * n * n); }
  const int high = L->boundary_condition.type == BC_DIRICHLET;      /* a face array holds the high domain face of its axis too */
  const size_t ni = (size_t)dense_extent(L->dim.i, high && layout == HPGMG_DENSE_FACE_I), nj = (size_t)dense_extent(L->dim.j, high && layout == HPGMG_DENSE_FACE_J);
  const int g = L->box_ghosts, dim = L->box_dim, jS = L->box_jStride, kS = L->box_kStride;
  double *box = (double *)malloc((size_t)L->box_volume * sizeof(double));
  int b, i, j, k, status = 0;
  for (b = 0; b < L->num_my_boxes; b++) {
    const box_type *B = &L->my_boxes[b];
    /* the high ghost layer along the array's axis belongs to it on the domain's high face (Dirichlet face arrays) */
    const int ei = dim + (ni > (size_t)L->dim.i && B->low.i + dim == L->dim.i);
    const int ej = dim + (nj > (size_t)L->dim.j && B->low.j + dim == L->dim.j);
    const int ek = dim + (dense_extent(L->dim.k, high && layout == HPGMG_DENSE_FACE_K) > L->dim.k && B->low.k + dim == L->dim.k);
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
static double *bnd_download(const double *src, size_t n) {
  double *h = (double *)malloc(n * sizeof(double));
  hpgmg_vector_download(h, src, n);
  return h;
}

/* mask, wall: hpgmg_dense_pack_lifted_faces (0, NULL: hpgmg_dense_pack_lifted); kappa: hpgmg_dense_pack_lifted_robin (NULL: the masked walls are Neumann) */
static int dense_pack_lifted_host(level_type *L, int id, const double *f, int where, const double *g, double b, int mask, const double *wall, const double *kappa) {
  if (!g || L->boundary_condition.type != BC_DIRICHLET) return -1;
  const int st = hpgmg_dense_pack(L, id, f, where, HPGMG_DENSE_CELL, HPGMG_DENSE_CHECK_FINITE);
  if (st < 0) return st;
  const int n = L->dim.i, g0 = L->box_ghosts, dim = L->box_dim, jS = L->box_jStride, kS = L->box_kStride;
  const double w = bnd_weight(b, L->h), wn = bnd_weight_neumann(b, L->h);
  double *gh = bnd_download(g, (size_t)6 * n * n), *wh = mask ? bnd_download(wall, (size_t)6 * n * n) : NULL;
  double *kh = mask && kappa ? bnd_download(kappa, (size_t)6 * n * n) : NULL;
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
        const int e = bnd_entry(n, face, gi, gj, gk);
        const double gv = gh[e];
        if (!isfinite(gv)) bad = 1;
        if ((mask >> face) & 1) T = T + (kh ? bnd_wall_phi(wn, wh[e], gv, kh[e], L->h) : (wn * wh[e]) * gv);
        else T = T + (w * bnd_beta(bi, bj, bk, face, ijk, jS, kS)) * gv;
        on = 1;
      }
      if (on) v[ijk] = v[ijk] + T;
    }
    hpgmg_vector_upload(B->vectors[id], v, (size_t)L->box_volume);
  }
  free(v); free(gh); free(wh); free(kh);
  return st | (bad ? HPGMG_DENSE_NOT_FINITE : 0);
}
__attribute__((weak)) int hpgmg_dense_pack_lifted(level_type *L, int id, const double *f, int where, const double *g, double b) {
  return dense_pack_lifted_host(L, id, f, where, g, b, 0, NULL, NULL);
}
__attribute__((weak)) int hpgmg_dense_pack_lifted_faces(level_type *L, int id, const double *f, int where, const double *g, double b, int mask, const double *wall) {
  if (mask < 0 || mask > 63 || (mask && !wall)) return -1;
  return dense_pack_lifted_host(L, id, f, where, g, b, mask, wall, NULL);
}
__attribute__((weak)) int hpgmg_dense_pack_lifted_robin(level_type *L, int id, const double *f, int where, const double *g, double b, int mask, const double *wall,
                                                        const double *kappa) {
  if (mask < 0 || mask > 63 || (mask && !wall)) return -1;
  return dense_pack_lifted_host(L, id, f, where, g, b, mask, wall, kappa);
}

static int boundary_flux_host(level_type *L, double *phi, const double *g, double b, int mask, const double *wall, const double *kappa) {
  const int n = L->dim.i, g0 = L->box_ghosts, dim = L->box_dim, jS = L->box_jStride, kS = L->box_kStride;
  const size_t len = (size_t)6 * n * n;
  const double w = bnd_weight(b, L->h), wn = bnd_weight_neumann(b, L->h);
  double *gh = bnd_download(g, len), *ph = (double *)calloc(len, sizeof(double)), *wh = mask ? bnd_download(wall, len) : NULL;
  double *kh = mask && kappa ? bnd_download(kappa, len) : NULL;
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
        if ((mask >> face) & 1) ph[e] = kh ? bnd_wall_phi(wn, wh[e], gh[e], kh[e], L->h) : (wn * wh[e]) * gh[e];
        else ph[e] = (w * bnd_beta(bi, bj, bk, face, ijk, jS, kS)) * gh[e];
      }
    }
  }
  hpgmg_vector_upload(phi, ph, len);
  free(bi); free(ph); free(gh); free(wh); free(kh);
  return bad ? HPGMG_DENSE_NOT_FINITE : 0;
}
__attribute__((weak)) int hpgmg_boundary_flux(level_type *L, double *phi, const double *g, double b) { return boundary_flux_host(L, phi, g, b, 0, NULL, NULL); }
__attribute__((weak)) int hpgmg_boundary_flux_faces(level_type *L, double *phi, const double *g, double b, int mask, const double *wall) {
  if (mask < 0 || mask > 63 || (mask && !wall)) return -1;
  return boundary_flux_host(L, phi, g, b, mask, wall, NULL);
}
__attribute__((weak)) int hpgmg_boundary_flux_robin(level_type *L, double *phi, const double *g, double b, int mask, const double *wall, const double *kappa) {
  if (mask < 0 || mask > 63 || (mask && !wall)) return -1;
  return boundary_flux_host(L, phi, g, b, mask, wall, kappa);
}

/* Robin walls (DESIGN.md §11.5) */
__attribute__((weak)) int hpgmg_boundary_check_kappa(level_type *L, const double *kappa, int where, int robin_mask, int *any_positive) {
  const int n = L->dim.i, len = 6 * n * n;
  int e, bits = 0;
  if (any_positive) *any_positive = 0;
  if (!kappa || robin_mask < 0 || robin_mask > 63 || (where != HPGMG_WHERE_HOST && where != HPGMG_WHERE_PLUGIN)) return -1;
  double *kh = where == HPGMG_WHERE_PLUGIN ? bnd_download(kappa, (size_t)len) : NULL;
  for (e = 0; e < len; e++) bits |= bnd_kappa_bits(n, robin_mask, e, kh ? kh[e] : kappa[e]);
  free(kh);
  if (any_positive) *any_positive = (bits & BND_KAPPA_POSITIVE) != 0;
  return bits & (HPGMG_DENSE_NOT_FINITE | HPGMG_DENSE_OUT_OF_RANGE);
}
__attribute__((weak)) void hpgmg_boundary_store_walls(level_type *L, const double *wall, const double *kappa, int mask) {
  const int n = L->dim.i, g0 = L->box_ghosts, dim = L->box_dim, jS = L->box_jStride, kS = L->box_kStride;
  const size_t len = (size_t)6 * n * n, vol = (size_t)L->box_volume;
  if (!mask || !wall) return;
  double *wh = bnd_download(wall, len), *kh = kappa ? bnd_download(kappa, len) : NULL;
  double *beta[3];
  int box, face, q, p;
  beta[0] = (double *)malloc(vol * 3 * sizeof(double)); beta[1] = beta[0] + vol; beta[2] = beta[1] + vol;
  for (box = 0; box < L->num_my_boxes; box++) {
    const box_type *B = &L->my_boxes[box];
    if (!bnd_box_on_domain_face(L, B)) continue;
    hpgmg_vector_download(beta[0], B->vectors[VECTOR_BETA_I], vol);
    hpgmg_vector_download(beta[1], B->vectors[VECTOR_BETA_J], vol);
    hpgmg_vector_download(beta[2], B->vectors[VECTOR_BETA_K], vol);
    for (face = 0; face < 6; face++) if ((mask >> face) & 1) for (q = 0; q < dim; q++) for (p = 0; p < dim; p++) {
      const int side = (face & 1) ? dim - 1 : 0;
      const int i = face < 2 ? side : p, j = face < 2 ? p : face < 4 ? side : q, k = face < 4 ? q : side;
      const int gi = B->low.i + i, gj = B->low.j + j, gk = B->low.k + k;
      if (!bnd_touches(n, face, gi, gj, gk)) continue;
      const int e = bnd_entry(n, face, gi, gj, gk), step = !(face & 1) ? 0 : face == 1 ? 1 : face == 3 ? jS : kS;
      beta[face >> 1][(i + g0) + (j + g0) * jS + (k + g0) * kS + step] = bnd_wall_beta(wh[e], kh ? kh[e] : 0.0, L->h);
    }
    hpgmg_vector_upload(B->vectors[VECTOR_BETA_I], beta[0], vol);
    hpgmg_vector_upload(B->vectors[VECTOR_BETA_J], beta[1], vol);
    hpgmg_vector_upload(B->vectors[VECTOR_BETA_K], beta[2], vol);
  }
  free(beta[0]); free(wh); free(kh);
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

/* D(c) of hpgmg_boundary_interp / _interp_faces / _interp_robin for fine cell (gi,gj,gk): u the coarse iterate as a dense (nc,nc,nc) array (read
 * only next to a masked wall: NULL with mask 0), hc the coarse h, kappa the coarse kappa array (NULL: the masked walls are Neumann) */
static double bnd_interp_delta(int nc, const double *g, const double *u, double hc, int mask, const double *kappa, int gi, int gj, int gk) {
  const bnd_p1_cell F = bnd_p1_of(gi, gj, gk);
  double D = 0.0, w;
  int t, q[3];
  for (t = 1; t < 8; t++) if (bnd_p1_ghost(nc, F, t, q, &w)) {
    const bnd_ghost G = bnd_ghost_faces(nc, g, hc, mask, kappa, q[0], q[1], q[2]);
    D = D + w * (G.needs_u ? G.c * u[((size_t)G.P[2] * nc + G.P[1]) * nc + G.P[0]] + G.s : G.s);
  }
  return D;
}

/* mask: hpgmg_boundary_interp_faces, which reads the coarse iterate next to a Neumann wall (0: hpgmg_boundary_interp) */
static void boundary_interp_host(level_type *Lf, int id, level_type *Lc, const double *g_c, int mask, const double *kappa_c) {
  const int n = Lf->dim.i, nc = Lc->dim.i, g0 = Lf->box_ghosts, dim = Lf->box_dim, jS = Lf->box_jStride, kS = Lf->box_kStride;
  double *gc = bnd_download(g_c, (size_t)6 * nc * nc), *v = (double *)malloc((size_t)Lf->box_volume * sizeof(double));
  double *uc = mask ? (double *)malloc((size_t)nc * nc * nc * sizeof(double)) : NULL;
  double *kc = mask && kappa_c ? bnd_download(kappa_c, (size_t)6 * nc * nc) : NULL;
  int box, i, j, k;
  if (uc) hpgmg_dense_unpack(Lc, id, uc, HPGMG_WHERE_HOST);
  for (box = 0; box < Lf->num_my_boxes; box++) {
    const box_type *B = &Lf->my_boxes[box];
    if (!bnd_box_on_domain_face(Lf, B)) continue;
    hpgmg_vector_download(v, B->vectors[id], (size_t)Lf->box_volume);
    for (k = 0; k < dim; k++) for (j = 0; j < dim; j++) for (i = 0; i < dim; i++) {
      const int gi = B->low.i + i, gj = B->low.j + j, gk = B->low.k + k, ijk = (i + g0) + (j + g0) * jS + (k + g0) * kS;
      if (gi > 0 && gj > 0 && gk > 0 && gi < n - 1 && gj < n - 1 && gk < n - 1) continue;
      v[ijk] = v[ijk] + bnd_interp_delta(nc, gc, uc, Lc->h, mask, kc, gi, gj, gk);
    }
    hpgmg_vector_upload(B->vectors[id], v, (size_t)Lf->box_volume);
  }
  free(uc); free(kc); free(v); free(gc);
}
__attribute__((weak)) void hpgmg_boundary_interp(level_type *Lf, int id, level_type *Lc, const double *g_c) { boundary_interp_host(Lf, id, Lc, g_c, 0, NULL); }
__attribute__((weak)) void hpgmg_boundary_interp_faces(level_type *Lf, int id, level_type *Lc, const double *g_c, int mask) { boundary_interp_host(Lf, id, Lc, g_c, mask, NULL); }
__attribute__((weak)) void hpgmg_boundary_interp_robin(level_type *Lf, int id, level_type *Lc, const double *g_c, int mask, const double *kappa_c) {
  boundary_interp_host(Lf, id, Lc, g_c, mask, kappa_c);
}

/* ------------------------------------------------------------------ face fluxes of a solution (include/hpgmg_operators.h; DESIGN.md §11.6)
 * q of the wall face `face` of the cell with value uc and wall entry e; beta: the level's beta on that face (read on a Dirichlet wall) */
static double flux_wall_host(int face, int e, double uc, double beta, double b, double wq, double h, int mask, const double *gh, const double *wh,
                             const double *kh, int *bad) {
  const double gv = gh ? gh[e] : 0.0;
  if (!isfinite(gv)) *bad = 1;
  if ((mask >> face) & 1) return bnd_flux_masked(b, wh[e], kh ? kh[e] : 0.0, h, uc, gv, face & 1);
  return bnd_flux_dirichlet(wq, beta, uc, gv, face & 1);
}
__attribute__((weak)) int hpgmg_dense_unpack_flux(level_type *L, int x_id, const double *g, double b, int mask, const double *wall, const double *kappa,
                                                  double *flux_i, double *flux_j, double *flux_k, int where) {
  if (L->num_ranks != 1 || x_id < 0 || x_id >= L->numVectors || !flux_i || !flux_j || !flux_k) return -1;
  if (where != HPGMG_WHERE_HOST && where != HPGMG_WHERE_PLUGIN) return -1;
  if (mask < 0 || mask > 63 || (mask && !wall) || L->dim.i != L->dim.j || L->dim.i != L->dim.k || L->box_ghosts < 1) return -1;
  const int walls = L->boundary_condition.type == BC_DIRICHLET;
  if (!walls && (g || mask)) return -1;
  const int n = L->dim.i, g0 = L->box_ghosts, dim = L->box_dim, jS = L->box_jStride, kS = L->box_kStride;
  const size_t len = (size_t)6 * n * n, vol = (size_t)L->box_volume;
  const size_t ni = (size_t)dense_extent(n, walls), nn = (size_t)n;      /* flux_i is (n, n, ni), flux_j (n, ni, n), flux_k (ni, n, n) */
  const double wq = bnd_weight_neumann(b, L->h), h = L->h;
  double *gh = g ? bnd_download(g, len) : NULL, *wh = mask ? bnd_download(wall, len) : NULL, *kh = mask && kappa ? bnd_download(kappa, len) : NULL;
  double *u = (double *)malloc(vol * 4 * sizeof(double)), *bi = u + vol, *bj = bi + vol, *bk = bj + vol;
  int box, i, j, k, bad = 0;
  for (box = 0; box < L->num_my_boxes; box++) {
    const box_type *B = &L->my_boxes[box];
    hpgmg_vector_download(u, B->vectors[x_id], vol);
    hpgmg_vector_download(bi, B->vectors[VECTOR_BETA_I], vol);
    hpgmg_vector_download(bj, B->vectors[VECTOR_BETA_J], vol);
    hpgmg_vector_download(bk, B->vectors[VECTOR_BETA_K], vol);
    for (k = 0; k < dim; k++) for (j = 0; j < dim; j++) for (i = 0; i < dim; i++) {
      const int gi = B->low.i + i, gj = B->low.j + j, gk = B->low.k + k, ijk = (i + g0) + (j + g0) * jS + (k + g0) * kS;
      const double uc = u[ijk];
      double *qi = flux_i + ((size_t)gk * nn + (size_t)gj) * ni + (size_t)gi, *qj = flux_j + ((size_t)gk * ni + (size_t)gj) * nn + (size_t)gi;
      double *qk = flux_k + ((size_t)gk * nn + (size_t)gj) * nn + (size_t)gi;
      if (walls && gi == 0) *qi = flux_wall_host(0, bnd_entry(n, 0, gi, gj, gk), uc, bi[ijk], b, wq, h, mask, gh, wh, kh, &bad);
      else *qi = bnd_flux_interior(wq, bi[ijk], u[ijk - 1], uc);
      if (walls && gi == n - 1) qi[1] = flux_wall_host(1, bnd_entry(n, 1, gi, gj, gk), uc, bi[ijk + 1], b, wq, h, mask, gh, wh, kh, &bad);
      if (walls && gj == 0) *qj = flux_wall_host(2, bnd_entry(n, 2, gi, gj, gk), uc, bj[ijk], b, wq, h, mask, gh, wh, kh, &bad);
      else *qj = bnd_flux_interior(wq, bj[ijk], u[ijk - jS], uc);
      if (walls && gj == n - 1) qj[nn] = flux_wall_host(3, bnd_entry(n, 3, gi, gj, gk), uc, bj[ijk + jS], b, wq, h, mask, gh, wh, kh, &bad);
      if (walls && gk == 0) *qk = flux_wall_host(4, bnd_entry(n, 4, gi, gj, gk), uc, bk[ijk], b, wq, h, mask, gh, wh, kh, &bad);
      else *qk = bnd_flux_interior(wq, bk[ijk], u[ijk - kS], uc);
      if (walls && gk == n - 1) qk[nn * nn] = flux_wall_host(5, bnd_entry(n, 5, gi, gj, gk), uc, bk[ijk + kS], b, wq, h, mask, gh, wh, kh, &bad);
    }
  }
  free(u); free(gh); free(wh); free(kh);
  return bad ? HPGMG_DENSE_NOT_FINITE : 0;
}

/* ------------------------------------------------------------------ coefficient sensitivities (include/hpgmg_operators.h; DESIGN.md §11.9)
 * G of the wall face `face` of the cell with state uc, adjoint lc and wall entry e */
static double sens_wall_host(int face, int e, double uc, double lc, double w, double wn, double h, int mask, const double *gh, const double *kh, int *bad) {
  const double gv = gh ? gh[e] : 0.0;
  if (!isfinite(gv)) *bad = 1;
  if ((mask >> face) & 1) return bnd_sens_masked(wn, kh ? kh[e] : 0.0, h, uc, gv, lc);
  return bnd_sens_dirichlet(w, uc, gv, lc);
}
__attribute__((weak)) int hpgmg_dense_unpack_sensitivity(level_type *L, int u_id, int lam_id, const double *g, double a, double b, int mask, const double *wall,
                                                         const double *kappa, double *d_alpha, double *d_beta_i, double *d_beta_j, double *d_beta_k, int where) {
  if (L->num_ranks != 1 || u_id < 0 || u_id >= L->numVectors || lam_id < 0 || lam_id >= L->numVectors || !d_beta_i || !d_beta_j || !d_beta_k) return -1;
  if (where != HPGMG_WHERE_HOST && where != HPGMG_WHERE_PLUGIN) return -1;
  if (mask < 0 || mask > 63 || (mask && !wall) || L->dim.i != L->dim.j || L->dim.i != L->dim.k || L->box_ghosts < 1) return -1;
  const int walls = L->boundary_condition.type == BC_DIRICHLET;
  if (!walls && (g || mask)) return -1;
  const int n = L->dim.i, g0 = L->box_ghosts, dim = L->box_dim, jS = L->box_jStride, kS = L->box_kStride;
  const size_t len = (size_t)6 * n * n, vol = (size_t)L->box_volume;
  const size_t ni = (size_t)dense_extent(n, walls), nn = (size_t)n;      /* d_beta_i is (n, n, ni), d_beta_j (n, ni, n), d_beta_k (ni, n, n) */
  const double w2 = bnd_sens_weight(b, L->h), w = bnd_weight(b, L->h), wn = bnd_weight_neumann(b, L->h), h = L->h;
  double *gh = g ? bnd_download(g, len) : NULL, *kh = mask && kappa ? bnd_download(kappa, len) : NULL;
  double *u = (double *)malloc(vol * 2 * sizeof(double)), *lam = u + vol;
  int box, i, j, k, bad = 0;
  for (box = 0; box < L->num_my_boxes; box++) {
    const box_type *B = &L->my_boxes[box];
    hpgmg_vector_download(u, B->vectors[u_id], vol);
    hpgmg_vector_download(lam, B->vectors[lam_id], vol);
    for (k = 0; k < dim; k++) for (j = 0; j < dim; j++) for (i = 0; i < dim; i++) {
      const int gi = B->low.i + i, gj = B->low.j + j, gk = B->low.k + k, ijk = (i + g0) + (j + g0) * jS + (k + g0) * kS;
      const double uc = u[ijk], lc = lam[ijk];
      const size_t cell = ((size_t)gk * nn + (size_t)gj) * nn + (size_t)gi;
      double *qi = d_beta_i + ((size_t)gk * nn + (size_t)gj) * ni + (size_t)gi, *qj = d_beta_j + ((size_t)gk * ni + (size_t)gj) * nn + (size_t)gi;
      double *qk = d_beta_k + cell;
      if (d_alpha) d_alpha[cell] = bnd_sens_alpha(a, uc, lc);
      if (walls && gi == 0) *qi = sens_wall_host(0, bnd_entry(n, 0, gi, gj, gk), uc, lc, w, wn, h, mask, gh, kh, &bad);
      else *qi = bnd_sens_interior(w2, u[ijk - 1], uc, lam[ijk - 1], lc);
      if (walls && gi == n - 1) qi[1] = sens_wall_host(1, bnd_entry(n, 1, gi, gj, gk), uc, lc, w, wn, h, mask, gh, kh, &bad);
      if (walls && gj == 0) *qj = sens_wall_host(2, bnd_entry(n, 2, gi, gj, gk), uc, lc, w, wn, h, mask, gh, kh, &bad);
      else *qj = bnd_sens_interior(w2, u[ijk - jS], uc, lam[ijk - jS], lc);
      if (walls && gj == n - 1) qj[nn] = sens_wall_host(3, bnd_entry(n, 3, gi, gj, gk), uc, lc, w, wn, h, mask, gh, kh, &bad);
      if (walls && gk == 0) *qk = sens_wall_host(4, bnd_entry(n, 4, gi, gj, gk), uc, lc, w, wn, h, mask, gh, kh, &bad);
      else *qk = bnd_sens_interior(w2, u[ijk - kS], uc, lam[ijk - kS], lc);
      if (walls && gk == n - 1) qk[nn * nn] = sens_wall_host(5, bnd_entry(n, 5, gi, gj, gk), uc, lc, w, wn, h, mask, gh, kh, &bad);
    }
  }
  free(u); free(gh); free(kh);
  return bad ? HPGMG_DENSE_NOT_FINITE : 0;
}

/* ------------------------------------------------------------------ cell-centred conductivities (include/hpgmg_operators.h; DESIGN.md §11.10)
 * The pack IS the face route: the three face arrays of means (include/hpgmg_boundary_math.h bnd_mean; a wall face its cell's own value), then the
 * existing packs.  The status is formed here, entry by entry and mean by mean: the existing packs' own check of a mean would call the mean of a
 * negative and a positive cell "not finite". */
static int cell_mean_refused(const level_type *L, const double *kcell, int where, int mean, int mask, const void *wall) {
  if (L->num_ranks != 1 || !kcell || L->dim.i != L->dim.j || L->dim.i != L->dim.k) return 1;
  if (where != HPGMG_WHERE_HOST && where != HPGMG_WHERE_PLUGIN) return 1;
  if (mean != HPGMG_MEAN_HARMONIC && mean != HPGMG_MEAN_ARITHMETIC) return 1;
  return mask < 0 || mask > 63 || (mask && (!wall || L->boundary_condition.type != BC_DIRICHLET));
}
__attribute__((weak)) int hpgmg_dense_pack_cell_mean(level_type *L, const double *kcell, int where, int mean, int mask, double *wall) {
  if (cell_mean_refused(L, kcell, where, mean, mask, wall)) return -1;
  const int n = L->dim.i, walls = L->boundary_condition.type == BC_DIRICHLET, ne = dense_extent(n, walls);
  const size_t nn = (size_t)n, cells = nn * nn * nn, len = nn * nn * (size_t)ne, ks[3] = { 1, nn, nn * nn };
  double *face = (double *)malloc(3 * len * sizeof(double));
  int axis, i, j, k, e, status = 0;
  size_t at;
  for (at = 0; at < cells; at++) status |= bnd_cell_bits(kcell[at]);
  for (axis = 0; axis < 3; axis++) {      /* the array of that axis is one longer along it when the level has walls: (n, n, ne), (n, ne, n), (ne, n, n) */
    const int ei = axis == 0 ? ne : n, ej = axis == 1 ? ne : n, ek = axis == 2 ? ne : n;
    double *F = face + axis * len;
    for (k = 0; k < ek; k++) for (j = 0; j < ej; j++) for (i = 0; i < ei; i++) {
      const int c = axis == 0 ? i : axis == 1 ? j : k;
      const size_t hi_at = ((size_t)k * nn + (size_t)j) * nn + (size_t)i;          /* the cell on the face's high side (c == n: there is none) */
      double *out = F + ((size_t)k * ej + (size_t)j) * ei + (size_t)i;
      if (walls && c == 0) *out = kcell[hi_at];
      else if (walls && c == n) *out = kcell[hi_at - ks[axis]];
      else {
        const double lo = c ? kcell[hi_at - ks[axis]] : kcell[hi_at + (nn - 1) * ks[axis]], hi = kcell[hi_at], m = bnd_mean(mean, lo, hi);
        status |= bnd_mean_bits(lo, hi, m);
        *out = m;
      }
    }
  }
  for (axis = 0; axis < 3; axis++) {
    const int id = axis == 0 ? VECTOR_BETA_I : axis == 1 ? VECTOR_BETA_J : VECTOR_BETA_K, layout = HPGMG_DENSE_FACE_I + axis;
    e = mask ? hpgmg_dense_pack_walls(L, id, face + axis * len, HPGMG_WHERE_HOST, layout, HPGMG_DENSE_CHECK_POSITIVE, mask, wall)
             : hpgmg_dense_pack(L, id, face + axis * len, HPGMG_WHERE_HOST, layout, HPGMG_DENSE_CHECK_POSITIVE);
    if (e < 0) { free(face); return -1; }
  }
  free(face);
  return status;
}

/* D G summed over the six faces of each cell in the written order; G as hpgmg_dense_unpack_sensitivity above forms it */
__attribute__((weak)) int hpgmg_dense_unpack_cell_sensitivity(level_type *L, int u_id, int lam_id, const double *kcell, int mean, const double *g, double a,
                                                              double b, int mask, const double *wall, const double *kappa, double *d_alpha, double *d_k,
                                                              int where) {
  if (L->num_ranks != 1 || u_id < 0 || u_id >= L->numVectors || lam_id < 0 || lam_id >= L->numVectors || !kcell || !d_k) return -1;
  if (where != HPGMG_WHERE_HOST && where != HPGMG_WHERE_PLUGIN) return -1;
  if (mean != HPGMG_MEAN_HARMONIC && mean != HPGMG_MEAN_ARITHMETIC) return -1;
  if (mask < 0 || mask > 63 || (mask && !wall) || L->dim.i != L->dim.j || L->dim.i != L->dim.k || L->box_ghosts < 1) return -1;
  const int walls = L->boundary_condition.type == BC_DIRICHLET;
  if (!walls && (g || mask)) return -1;
  const int n = L->dim.i, g0 = L->box_ghosts, dim = L->box_dim, jS = L->box_jStride, kS = L->box_kStride;
  const size_t len = (size_t)6 * n * n, vol = (size_t)L->box_volume, nn = (size_t)n;
  const double w2 = bnd_sens_weight(b, L->h), w = bnd_weight(b, L->h), wn = bnd_weight_neumann(b, L->h), h = L->h;
  double *gh = g ? bnd_download(g, len) : NULL, *kh = mask && kappa ? bnd_download(kappa, len) : NULL;
  double *u = (double *)malloc(vol * 2 * sizeof(double)), *lam = u + vol;
  int box, i, j, k, axis, bad = 0, status = 0;
  for (box = 0; box < L->num_my_boxes; box++) {
    const box_type *B = &L->my_boxes[box];
    hpgmg_vector_download(u, B->vectors[u_id], vol);
    hpgmg_vector_download(lam, B->vectors[lam_id], vol);
    for (k = 0; k < dim; k++) for (j = 0; j < dim; j++) for (i = 0; i < dim; i++) {
      const int gc[3] = { B->low.i + i, B->low.j + j, B->low.k + k }, ijk = (i + g0) + (j + g0) * jS + (k + g0) * kS, vs[3] = { 1, jS, kS };
      const size_t cell = ((size_t)gc[2] * nn + (size_t)gc[1]) * nn + (size_t)gc[0], ks[3] = { 1, nn, nn * nn };
      const double uc = u[ijk], lc = lam[ijk], kc = kcell[cell];
      double GD[6];
      status |= bnd_cell_bits(kc);
      for (axis = 0; axis < 3; axis++) {
        if (walls && gc[axis] == 0) GD[2 * axis] = sens_wall_host(2 * axis, bnd_entry(n, 2 * axis, gc[0], gc[1], gc[2]), uc, lc, w, wn, h, mask, gh, kh, &bad);          /* D = 1.0 */
        else {
          const double klo = gc[axis] ? kcell[cell - ks[axis]] : kcell[cell + (nn - 1) * ks[axis]];
          status |= bnd_mean_bits(klo, kc, bnd_mean(mean, klo, kc));          /* each mean once: by the cell on its high side */
          GD[2 * axis] = bnd_sens_interior(w2, u[ijk - vs[axis]], uc, lam[ijk - vs[axis]], lc) * bnd_mean_dhi(mean, klo, kc);
        }
        if (walls && gc[axis] == n - 1) GD[2 * axis + 1] = sens_wall_host(2 * axis + 1, bnd_entry(n, 2 * axis + 1, gc[0], gc[1], gc[2]), uc, lc, w, wn, h, mask, gh, kh, &bad);          /* D = 1.0 */
        else {
          const double khi = gc[axis] < n - 1 ? kcell[cell + ks[axis]] : kcell[cell - (nn - 1) * ks[axis]];
          GD[2 * axis + 1] = bnd_sens_interior(w2, uc, u[ijk + vs[axis]], lc, lam[ijk + vs[axis]]) * bnd_mean_dlo(mean, kc, khi);
        }
      }
      if (d_alpha) d_alpha[cell] = bnd_sens_alpha(a, uc, lc);
      d_k[cell] = ((((GD[0] + GD[1]) + GD[2]) + GD[3]) + GD[4]) + GD[5];
    }
  }
  free(u); free(gh); free(kh);
  return status | (bad ? HPGMG_DENSE_NOT_FINITE : 0);
}

/* ------------------------------------------------------------------ the implicit time march (include/hpgmg_operators.h; DESIGN.md §11.8)
 * The two cell expressions of include/hpgmg_step_math.h over the interior cells, box by box; weak like the dense pair above (the HIP plugin:
 * host/plugin_step.c).  A box goes up whole, so a vector that is only written (u_old) is downloaded first: its ghost and padding cells keep
 * their content. */
static double *step_boxes(const level_type *L, int n) {      /* room for n padded boxes */
  double *v = (double *)malloc((size_t)n * (size_t)L->box_volume * sizeof(double));
  if (!v) { fprintf(stderr, "hpgmg: time march: no memory for %d boxes of %d doubles\n", n, L->box_volume); abort(); }
  return v;
}
__attribute__((weak)) void hpgmg_step_rhs(level_type *L, int F_id, int u_id, int uold_id, int w_id, double a, double c) {
  const int g = L->box_ghosts, dim = L->box_dim, jS = L->box_jStride, kS = L->box_kStride;
  const size_t vol = (size_t)L->box_volume;
  double *v = step_boxes(L, 5), *F = v, *al = v + vol, *u = v + 2 * vol, *w = v + 3 * vol, *uold = v + 4 * vol;
  int bx, i, j, k;
  for (bx = 0; bx < L->num_my_boxes; bx++) {
    const box_type *B = &L->my_boxes[bx];
    hpgmg_vector_download(F, B->vectors[F_id], vol); hpgmg_vector_download(al, B->vectors[VECTOR_ALPHA], vol);
    hpgmg_vector_download(u, B->vectors[u_id], vol); hpgmg_vector_download(w, B->vectors[w_id], vol);
    hpgmg_vector_download(uold, B->vectors[uold_id], vol);
    for (k = 0; k < dim; k++) for (j = 0; j < dim; j++) for (i = 0; i < dim; i++) {
      const int ijk = (i + g) + (j + g) * jS + (k + g) * kS;
      F[ijk] = step_rhs_cell(F[ijk], al[ijk], u[ijk], w[ijk], a, c);
      uold[ijk] = u[ijk];
    }
    hpgmg_vector_upload(B->vectors[F_id], F, vol); hpgmg_vector_upload(B->vectors[uold_id], uold, vol);
  }
  free(v);
}
__attribute__((weak)) void hpgmg_step_rate(level_type *L, int w_id, int r_id, int u_id, int uold_id, double a, double c, double *max_abs) {
  const int g = L->box_ghosts, dim = L->box_dim, jS = L->box_jStride, kS = L->box_kStride;
  const size_t vol = (size_t)L->box_volume;
  double *v = step_boxes(L, 5), *w = v, *al = v + vol, *r = v + 2 * vol, *u = v + 3 * vol, *uold = v + 4 * vol;
  double best = 0.0;
  int bx, i, j, k;
  for (bx = 0; bx < L->num_my_boxes; bx++) {
    const box_type *B = &L->my_boxes[bx];
    hpgmg_vector_download(w, B->vectors[w_id], vol); hpgmg_vector_download(al, B->vectors[VECTOR_ALPHA], vol);
    hpgmg_vector_download(r, B->vectors[r_id], vol); hpgmg_vector_download(u, B->vectors[u_id], vol);
    hpgmg_vector_download(uold, B->vectors[uold_id], vol);
    for (k = 0; k < dim; k++) for (j = 0; j < dim; j++) for (i = 0; i < dim; i++) {
      const int ijk = (i + g) + (j + g) * jS + (k + g) * kS;
      w[ijk] = step_rate_cell(r[ijk], al[ijk], u[ijk], uold[ijk], w[ijk], a, c);
      const double f = fabs(w[ijk]);
      if (f > best) best = f;
    }
    hpgmg_vector_upload(B->vectors[w_id], w, vol);
  }
  free(v);
  *max_abs = best;
}

/* ------------------------------------------------------------------ the CG passes: portable forms (include/hpgmg_operators.h; DESIGN.md §11.3)
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

/* ------------------------------------------------------------------ block linear algebra: portable forms (include/hpgmg_operators.h; DESIGN.md §11.11)
 * The CG passes' one order for every Gram entry (pcg_leaves / pcg_fold above), the combination and the residuals cell by cell, from downloaded boxes.
 * Weak like the CG passes: the HIP plugin (host/plugin_block.c) replaces them with kernels/block.hip and comes back to these on a level those do not take. */
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
static double *block_download(const level_type *L, int id) {      /* every box of one vector, whole */
  const size_t vol = (size_t)L->box_volume;
  double *v = (double *)malloc((size_t)L->num_my_boxes * vol * sizeof(double));
  int bx;
  for (bx = 0; bx < L->num_my_boxes; bx++) hpgmg_vector_download(v + (size_t)bx * vol, L->my_boxes[bx].vectors[id], vol);
  return v;
}
int hpgmg_block_gram_host(level_type *L, const int *a_ids, int na, const int *b_ids, int nb, int w_id, double *G) {
  const size_t vol = (size_t)L->box_volume, len = (size_t)L->num_my_boxes * vol;
  int i, j, bx, same = (na == nb);
  size_t q;
  if (!G || !block_ids_ok(L, a_ids, na, HPGMG_BLOCK_MAX_IN) || !block_ids_ok(L, b_ids, nb, HPGMG_BLOCK_MAX_IN) || w_id >= L->numVectors) return -1;
  for (i = 0; same && i < na; i++) same = (a_ids[i] == b_ids[i]);
  double *w = w_id >= 0 ? block_download(L, w_id) : NULL;
  for (i = 0; i < na; i++) {
    double *va = block_download(L, a_ids[i]);
    if (w) for (q = 0; q < len; q++) va[q] = w[q] * va[q];       /* the leaf term is (w * a) * b */
    for (j = 0; j < nb; j++) {
      if (same && j < i) { G[i * nb + j] = G[j * nb + i]; continue; }
      double *vb = block_download(L, b_ids[j]);
      pcg_leaves P = pcg_leaves_of(L);
      for (bx = 0; bx < L->num_my_boxes; bx++) pcg_box_leaves(L, &P, bx, va + (size_t)bx * vol, vb + (size_t)bx * vol);
      G[i * nb + j] = pcg_fold(&P);
      free(vb);
    }
    free(va);
  }
  free(w);
  return 0;
}
int hpgmg_block_combine_host(level_type *L, const int *out_ids, int nout, const int *in_ids, int nin, const double *C) {
  const int g = L->box_ghosts, dim = L->box_dim, jS = L->box_jStride, kS = L->box_kStride;
  const size_t vol = (size_t)L->box_volume;
  int bx, i, j, k, p, q;
  if (!C || !block_ids_ok(L, out_ids, nout, HPGMG_BLOCK_MAX_OUT) || !block_ids_ok(L, in_ids, nin, HPGMG_BLOCK_MAX_IN) || !block_ids_distinct(out_ids, nout)) return -1;
  double *in = (double *)malloc((size_t)(nin + nout) * vol * sizeof(double)), *out = in + (size_t)nin * vol;
  for (bx = 0; bx < L->num_my_boxes; bx++) {
    const box_type *B = &L->my_boxes[bx];
    for (p = 0; p < nin; p++) hpgmg_vector_download(in + (size_t)p * vol, B->vectors[in_ids[p]], vol);
    for (q = 0; q < nout; q++) hpgmg_vector_download(out + (size_t)q * vol, B->vectors[out_ids[q]], vol);      /* a box goes up whole: ghosts and padding keep their content */
    for (k = 0; k < dim; k++) for (j = 0; j < dim; j++) for (i = 0; i < dim; i++) {
      const int ijk = (i + g) + (j + g) * jS + (k + g) * kS;
      for (q = 0; q < nout; q++) {
        double chain = 0.0;
        for (p = 0; p < nin; p++) { const double t = C[p * nout + q] * in[(size_t)p * vol + ijk]; chain = chain + t; }
        out[(size_t)q * vol + ijk] = chain;
      }
    }
    for (q = 0; q < nout; q++) hpgmg_vector_upload(B->vectors[out_ids[q]], out + (size_t)q * vol, vol);
  }
  free(in);
  return 0;
}
int hpgmg_block_residual_host(level_type *L, const int *r_ids, const int *ax_ids, const int *x_ids, int n, int w_id, const double *mu, double *rmax,
                              double *mxmax) {
  const int g = L->box_ghosts, dim = L->box_dim, jS = L->box_jStride, kS = L->box_kStride;
  const size_t vol = (size_t)L->box_volume;
  int bx, i, j, k, q;
  if (!mu || !rmax || !mxmax || !block_ids_ok(L, r_ids, n, HPGMG_BLOCK_MAX_OUT) || !block_ids_ok(L, ax_ids, n, HPGMG_BLOCK_MAX_OUT) ||
      !block_ids_ok(L, x_ids, n, HPGMG_BLOCK_MAX_OUT) || !block_ids_distinct(r_ids, n) || w_id >= L->numVectors) return -1;
  for (q = 0; q < n; q++) for (i = 0; i < n; i++) if (i != q && (r_ids[q] == ax_ids[i] || r_ids[q] == x_ids[i])) return -1;      /* r_q may alias its own column only */
  if (w_id >= 0) for (q = 0; q < n; q++) if (r_ids[q] == w_id) return -1;
  double *v = (double *)malloc(4 * vol * sizeof(double)), *r = v, *ax = v + vol, *x = v + 2 * vol, *w = v + 3 * vol;
  for (q = 0; q < n; q++) rmax[q] = mxmax[q] = 0.0;
  for (bx = 0; bx < L->num_my_boxes; bx++) {
    const box_type *B = &L->my_boxes[bx];
    if (w_id >= 0) hpgmg_vector_download(w, B->vectors[w_id], vol);
    for (q = 0; q < n; q++) {
      hpgmg_vector_download(r, B->vectors[r_ids[q]], vol); hpgmg_vector_download(ax, B->vectors[ax_ids[q]], vol); hpgmg_vector_download(x, B->vectors[x_ids[q]], vol);
      for (k = 0; k < dim; k++) for (j = 0; j < dim; j++) for (i = 0; i < dim; i++) {
        const int ijk = (i + g) + (j + g) * jS + (k + g) * kS;
        const double mx = w_id >= 0 ? w[ijk] * x[ijk] : x[ijk], t = mu[q] * mx;
        r[ijk] = ax[ijk] - t;
        const double fr = fabs(r[ijk]), fm = fabs(mx);
        if (fr > rmax[q]) rmax[q] = fr;
        if (fm > mxmax[q]) mxmax[q] = fm;
      }
      hpgmg_vector_upload(B->vectors[r_ids[q]], r, vol);
    }
  }
  free(v);
  return 0;
}
__attribute__((weak)) int hpgmg_block_gram(level_type *L, const int *a_ids, int na, const int *b_ids, int nb, int w_id, double *G) { return hpgmg_block_gram_host(L, a_ids, na, b_ids, nb, w_id, G); }
__attribute__((weak)) int hpgmg_block_combine(level_type *L, const int *out_ids, int nout, const int *in_ids, int nin, const double *C) { return hpgmg_block_combine_host(L, out_ids, nout, in_ids, nin, C); }
__attribute__((weak)) int hpgmg_block_residual(level_type *L, const int *r_ids, const int *ax_ids, const int *x_ids, int n, int w_id, const double *mu, double *rmax, double *mxmax) {
  return hpgmg_block_residual_host(L, r_ids, ax_ids, x_ids, n, w_id, mu, rmax, mxmax);
}


/* ------------------------------------------------------------------ the Newmark march: portable forms (include/hpgmg_operators.h; DESIGN.md §11.12)
 * The cell expressions of include/hpgmg_wave_math.h over the interior cells, box by box through download / upload (a box goes up whole, so a vector that
 * is only written is downloaded first: its ghost and padding doubles keep their content), and the two sums in the CG passes' one order (pcg_leaves /
 * pcg_fold above) from per-cell leaf terms.  Weak like the block hooks: the HIP plugin (host/plugin_wave.c) replaces them with kernels/dense_wave.hip and
 * comes back to these on a level those do not take. */
static void wave_box_leaves(const level_type *L, pcg_leaves *P, int bx, const double *term) {      /* pcg_box_leaves with the terms already formed */
  const int g = L->box_ghosts, dim = L->box_dim, jS = L->box_jStride, kS = L->box_kStride;
  int i, j, k;
  size_t s;
  for (s = 0; s < P->S; s++) for (j = 0; j < dim; j++) for (i = 0; i < dim; i++) {
    const int k1 = (int)(s + 1) * HPGMG_PCG_SEGMENT < dim ? (int)(s + 1) * HPGMG_PCG_SEGMENT : dim;
    double chain = 0.0;
    for (k = (int)s * HPGMG_PCG_SEGMENT; k < k1; k++) chain = chain + term[(i + g) + (j + g) * jS + (k + g) * kS];
    P->V[(size_t)(i + dim * j) + P->W * (s + P->S * (size_t)bx)] = chain;
  }
}
int hpgmg_wave_predict_host(level_type *L, int u_id, int uold_id, int v_id, int F_id, int q_id, double dt, double cu, double cv, double a, double sigma) {
  const int g = L->box_ghosts, dim = L->box_dim, jS = L->box_jStride, kS = L->box_kStride, ids[5] = { u_id, uold_id, v_id, F_id, q_id };
  const size_t vol = (size_t)L->box_volume;
  int bx, i, j, k;
  if (wave_ids_refused(ids, 4, 5, L->numVectors, VECTOR_ALPHA)) return -1;
  double *w = step_boxes(L, 6), *u = w, *uold = w + vol, *v = w + 2 * vol, *F = w + 3 * vol, *q = w + 4 * vol, *al = w + 5 * vol;
  for (bx = 0; bx < L->num_my_boxes; bx++) {
    const box_type *B = &L->my_boxes[bx];
    hpgmg_vector_download(u, B->vectors[u_id], vol); hpgmg_vector_download(uold, B->vectors[uold_id], vol); hpgmg_vector_download(v, B->vectors[v_id], vol);
    hpgmg_vector_download(F, B->vectors[F_id], vol); hpgmg_vector_download(q, B->vectors[q_id], vol); hpgmg_vector_download(al, B->vectors[VECTOR_ALPHA], vol);
    for (k = 0; k < dim; k++) for (j = 0; j < dim; j++) for (i = 0; i < dim; i++) {
      const int ijk = (i + g) + (j + g) * jS + (k + g) * kS;
      const double ut = wave_ut_cell(u[ijk], v[ijk], q[ijk], dt, cu), vt = wave_vt_cell(v[ijk], q[ijk], cv);
      F[ijk] = wave_rhs_cell(F[ijk], al[ijk], ut, vt, a, sigma);
      u[ijk] = ut; uold[ijk] = ut; v[ijk] = vt;
    }
    hpgmg_vector_upload(B->vectors[u_id], u, vol); hpgmg_vector_upload(B->vectors[uold_id], uold, vol);
    hpgmg_vector_upload(B->vectors[v_id], v, vol); hpgmg_vector_upload(B->vectors[F_id], F, vol);
  }
  free(w);
  return 0;
}
int hpgmg_wave_correct_host(level_type *L, int q_id, int v_id, int u_id, int uold_id, int F_id, int r_id, double a, double cq, double cg, double sums[2]) {
  const int g = L->box_ghosts, dim = L->box_dim, jS = L->box_jStride, kS = L->box_kStride, ids[6] = { q_id, v_id, u_id, uold_id, F_id, r_id };
  const size_t vol = (size_t)L->box_volume;
  int bx, i, j, k;
  if (!sums || wave_ids_refused(ids, 2, 6, L->numVectors, VECTOR_ALPHA)) return -1;
  double *w = step_boxes(L, 9), *q = w, *v = w + vol, *u = w + 2 * vol, *uold = w + 3 * vol, *F = w + 4 * vol, *r = w + 5 * vol, *al = w + 6 * vol;
  double *kin = w + 7 * vol, *pot = w + 8 * vol;
  pcg_leaves K = pcg_leaves_of(L), U = pcg_leaves_of(L);
  for (bx = 0; bx < L->num_my_boxes; bx++) {
    const box_type *B = &L->my_boxes[bx];
    hpgmg_vector_download(q, B->vectors[q_id], vol); hpgmg_vector_download(v, B->vectors[v_id], vol); hpgmg_vector_download(u, B->vectors[u_id], vol);
    hpgmg_vector_download(uold, B->vectors[uold_id], vol); hpgmg_vector_download(F, B->vectors[F_id], vol); hpgmg_vector_download(r, B->vectors[r_id], vol);
    hpgmg_vector_download(al, B->vectors[VECTOR_ALPHA], vol);
    for (k = 0; k < dim; k++) for (j = 0; j < dim; j++) for (i = 0; i < dim; i++) {
      const int ijk = (i + g) + (j + g) * jS + (k + g) * kS;
      q[ijk] = wave_q_cell(u[ijk], uold[ijk], cq);
      v[ijk] = wave_v_cell(v[ijk], q[ijk], cg);
      kin[ijk] = wave_kinetic_cell(al[ijk], v[ijk]);
      pot[ijk] = wave_potential_cell(u[ijk], F[ijk], r[ijk], al[ijk], a);
    }
    wave_box_leaves(L, &K, bx, kin); wave_box_leaves(L, &U, bx, pot);
    hpgmg_vector_upload(B->vectors[q_id], q, vol); hpgmg_vector_upload(B->vectors[v_id], v, vol);
  }
  free(w);
  sums[0] = pcg_fold(&K); sums[1] = pcg_fold(&U);
  return 0;
}
int hpgmg_wave_init_host(level_type *L, int q_id, int r_id, int u_id, int v_id, int F_id, double a, double sigma, double sums[2]) {
  const int g = L->box_ghosts, dim = L->box_dim, jS = L->box_jStride, kS = L->box_kStride, ids[5] = { q_id, r_id, u_id, v_id, F_id };
  const size_t vol = (size_t)L->box_volume;
  int bx, i, j, k;
  if (!sums || wave_ids_refused(ids, 1, 5, L->numVectors, VECTOR_ALPHA)) return -1;
  double *w = step_boxes(L, 8), *q = w, *r = w + vol, *u = w + 2 * vol, *v = w + 3 * vol, *F = w + 4 * vol, *al = w + 5 * vol, *kin = w + 6 * vol, *pot = w + 7 * vol;
  pcg_leaves K = pcg_leaves_of(L), U = pcg_leaves_of(L);
  for (bx = 0; bx < L->num_my_boxes; bx++) {
    const box_type *B = &L->my_boxes[bx];
    hpgmg_vector_download(q, B->vectors[q_id], vol); hpgmg_vector_download(r, B->vectors[r_id], vol); hpgmg_vector_download(u, B->vectors[u_id], vol);
    hpgmg_vector_download(v, B->vectors[v_id], vol); hpgmg_vector_download(F, B->vectors[F_id], vol); hpgmg_vector_download(al, B->vectors[VECTOR_ALPHA], vol);
    for (k = 0; k < dim; k++) for (j = 0; j < dim; j++) for (i = 0; i < dim; i++) {
      const int ijk = (i + g) + (j + g) * jS + (k + g) * kS;
      q[ijk] = wave_init_cell(r[ijk], al[ijk], u[ijk], v[ijk], a, sigma);
      kin[ijk] = wave_kinetic_cell(al[ijk], v[ijk]);
      pot[ijk] = wave_potential_cell(u[ijk], F[ijk], r[ijk], al[ijk], a);
    }
    wave_box_leaves(L, &K, bx, kin); wave_box_leaves(L, &U, bx, pot);
    hpgmg_vector_upload(B->vectors[q_id], q, vol);
  }
  free(w);
  sums[0] = pcg_fold(&K); sums[1] = pcg_fold(&U);
  return 0;
}
__attribute__((weak)) int hpgmg_wave_predict(level_type *L, int u_id, int uold_id, int v_id, int F_id, int q_id, double dt, double cu, double cv, double a, double sigma) {
  return hpgmg_wave_predict_host(L, u_id, uold_id, v_id, F_id, q_id, dt, cu, cv, a, sigma);
}
__attribute__((weak)) int hpgmg_wave_correct(level_type *L, int q_id, int v_id, int u_id, int uold_id, int F_id, int r_id, double a, double cq, double cg, double sums[2]) {
  return hpgmg_wave_correct_host(L, q_id, v_id, u_id, uold_id, F_id, r_id, a, cq, cg, sums);
}
__attribute__((weak)) int hpgmg_wave_init(level_type *L, int q_id, int r_id, int u_id, int v_id, int F_id, double a, double sigma, double sums[2]) {
  return hpgmg_wave_init_host(L, q_id, r_id, u_id, v_id, F_id, a, sigma, sums);
}
