/*
 * plugin_pairs.c -- smooth() as fused sweep pairs (kernels/cheby_pair.hpp): the fp32 coefficient copies, the Dinv record, the pairs' private vectors, the Chebyshev and GSRB pairs, interpolation_vcycle folded into the first pair.
 * Part of the operator plugin (see operators_hip.c); no arithmetic on vector data happens here.
 */
#include "plugin_internal.h"

/* BASELINE config 5: mixed-precision Chebyshev smoother.  32 = the fused sweep pairs read fp32 copies of the five
 * coefficient vectors (the iterate, the right-hand side and all arithmetic stay fp64; residual, restriction,
 * interpolation and every level the pair kernel does not cover are unchanged).  64 (default) = bit-exact fp64. */
void hpgmg_set_smoother_precision(int bits) { hp_switch_set(SW_SMOOTHER_PRECISION, (bits == 32) ? 32 : 64); }
int hpgmg_get_smoother_precision(void) {
  return hp_switch(SW_SMOOTHER_PRECISION) == 32 ? 32 : 64;
}
static const float *const *coef32_of(level_type *L) {
  backend_t *B = hp_backend_of(L);
  if (hpgmg_get_smoother_precision() != 32) return NULL;
  if (!B->coef32) {
    int bx;
    float **base = (float **)calloc((size_t)L->num_my_boxes, sizeof(float *));
    B->coef32 = (float *)hpgmg_hip_malloc(((size_t)L->num_my_boxes * 5 * (size_t)L->box_volume + 4) * sizeof(float));
    B->d_coef32_base = (float **)hpgmg_hip_malloc((size_t)L->num_my_boxes * sizeof(float *));
    if (!B->coef32 || !B->d_coef32_base) { fprintf(stderr, "hpgmg: no memory for the fp32 coefficient copies\n"); abort(); }
    /* pairs (2 floats) must be 8-byte aligned where the fp64 pairs are 16-byte aligned: same parity of the first interior cell */
    const size_t pad = ((uintptr_t)L->my_boxes[0].vectors[0] % 16) / sizeof(double);
    for (bx = 0; bx < L->num_my_boxes; bx++) base[bx] = B->coef32 + pad + (size_t)bx * 5 * (size_t)L->box_volume;
    HIP_OK(hpgmg_hip_memcpy_h2d(B->d_coef32_base, base, (size_t)L->num_my_boxes * sizeof(float *)));
    free(base);
    B->coef32_valid = 0;
  }
  if (!B->coef32_valid) { HIP_OK(hpgmg_hip_coef32_refresh(&B->dev, (float *const *)B->d_coef32_base, L->numVectors)); B->coef32_valid = 1; }
  return (const float *const *)B->d_coef32_base;
}
void hp_coef32_invalidate(level_type *L) { backend_t *B = hp_backend_of(L); B->coef32_valid = 0; hp_dinv_record_clear(L); if (B->halo) B->halo->coef_valid = 0; hp_images_invalidate_coefficients(B); hpgmg_hip_pair_packed_invalidate(&B->dev); }

/* ---- the record "VECTOR_DINV is rebuild_operator's" (plugin_internal.h: backend_t.dinv_rebuilt).  The levels that hold it are listed, so that a raw copy into
 * device storage (hpgmg_vector_upload / _copy know a pointer, not a level) can find the level it touches; a level the list has no room for never gets the record. */
enum { DINV_RECORDS = 64 };
static level_type *dinv_recorded[DINV_RECORDS];
void hp_dinv_record_forget(level_type *L) { int q; for (q = 0; q < DINV_RECORDS; q++) if (dinv_recorded[q] == L) dinv_recorded[q] = NULL; }
void hp_dinv_record_clear(level_type *L) {
  hpgmg_level_ext *X = hpgmg_level_ext_get(L);
  if (X->backend) { ((backend_t *)X->backend)->dinv_rebuilt = 0; ((backend_t *)X->backend)->alpha_uniform = 0; }
  hp_dinv_record_forget(L);
}
void hp_dinv_record_set(level_type *L, double a, double b, double h2inv) {
  backend_t *B = hp_backend_of(L);
  int q, slot = -1;
  for (q = 0; q < DINV_RECORDS; q++) { if (dinv_recorded[q] == L) { slot = q; break; } if (slot < 0 && !dinv_recorded[q]) slot = q; }
  if (slot < 0) return;
  dinv_recorded[slot] = L;
  B->dinv_rebuilt = 1; B->dinv_a = a; B->dinv_b = b; B->dinv_h2inv = h2inv;
}
void hp_dinv_record_written(const double *dst, size_t n) {
  int q, bx;
  for (q = 0; q < DINV_RECORDS; q++) {
    level_type *L = dinv_recorded[q];
    if (!L) continue;
    for (bx = 0; bx < L->num_my_boxes; bx++) {
      const double *lo = L->my_boxes[bx].vectors[0] + (size_t)VECTOR_DINV * (size_t)L->box_volume, *hi = L->my_boxes[bx].vectors[0] + (size_t)(VECTOR_ALPHA + 1) * (size_t)L->box_volume;
      if (dst < hi && dst + n > lo) { hp_dinv_record_clear(L); break; }
    }
  }
}
/* may this launch form Dinv?  The record holds, it was made with exactly these a, b, h2inv (bit for bit), and the switch is on; the kernel library adds: an instance that can */
void hpgmg_set_pair_form_dinv(int on) { hp_switch_set(SW_PAIR_FORM_DINV, on ? 1 : 0); }
long long hpgmg_pair_formed_dinv_launches(void) { hp_lazy_flush(); return hpgmg_hip_pair_formed_dinv_launches(); }
static int dinv_formable(const backend_t *B, double a, double b, double h2inv) {
  return hp_switch(SW_PAIR_FORM_DINV) && B->dinv_rebuilt && memcmp(&a, &B->dinv_a, sizeof a) == 0 && memcmp(&b, &B->dinv_b, sizeof b) == 0 && memcmp(&h2inv, &B->dinv_h2inv, sizeof h2inv) == 0;
}

/* ---- the record "alpha is one bit pattern" (plugin_internal.h: backend_t.alpha_uniform).  It lives inside the Dinv record's lifetime: made only where that record was just
 * set, gone with it.  One rank for now: the decision would be safe per rank, but no multi-rank instance takes it. */
void hpgmg_set_uniform_alpha(int on) { hp_switch_set(SW_UNIFORM_ALPHA, on ? 1 : 0); }
long long hpgmg_uniform_alpha_launches(void) { hp_lazy_flush(); return hpgmg_hip_pair_uniform_alpha_launches() + hpgmg_hip_stencil_uniform_alpha_launches(); }
void hp_alpha_record_check(level_type *L) {
  backend_t *B = hp_backend_of(L);
  int uniform = 0; double value = 0.0;
  B->alpha_uniform = 0;
  if (!B->dinv_rebuilt || !B->all_faces_local || L->num_my_boxes < 1) return;      /* a level that got no Dinv record gets none */
  BLAS1(hpgmg_hip_vector_uniform(&B->dev, VECTOR_ALPHA, &uniform, &value));
  B->alpha_uniform = uniform; B->alpha_value = value;
}
static int alpha_uniform_usable(const backend_t *B) { return hp_switch(SW_UNIFORM_ALPHA) && B->dinv_rebuilt && B->alpha_uniform && B->all_faces_local; }
int hp_alpha_uniform_arm_residual(const backend_t *B) {
  if (!alpha_uniform_usable(B) || hp_variant() != HPGMG_HIP_7PT_VC_HELMHOLTZ) return 0;
  hpgmg_hip_stencil_uniform_alpha(B->alpha_value);
  return 1;
}

static long long pair_remote_smooths = 0, fp32_pair_smooths = 0;
long long hpgmg_pair_remote_smooths(void) { return pair_remote_smooths; }   /* smooth() calls done as sweep pairs with remote faces (tests) */
long long hpgmg_fp32_pair_smooths(void) { hp_lazy_flush(); return fp32_pair_smooths; }      /* smooth() calls whose sweep pairs read the fp32 coefficient copies (tests; a postponed smooth() is issued first) */

/* the two plugin-private vectors per box that hold x1, x2 of the first sweep pair of a smooth() */
void hp_ensure_pair_scratch(level_type *L, backend_t *B) {
  if (!B->pair_scratch) {
    int bx;
    double **base = (double **)calloc((size_t)L->num_my_boxes, sizeof(double *));
    B->pair_scratch = (double *)hpgmg_hip_malloc(((size_t)L->num_my_boxes * 2 * (size_t)L->box_volume + 2) * sizeof(double));
    B->d_pair_base = (double **)hpgmg_hip_malloc((size_t)L->num_my_boxes * sizeof(double *));
    if (!B->pair_scratch || !B->d_pair_base) { fprintf(stderr, "hpgmg: no memory for the sweep-pair scratch vectors\n"); abort(); }
    /* the vector bases share the level's alignment class so the first interior cell is 16-byte aligned here too */
    const size_t pad = ((uintptr_t)L->my_boxes[0].vectors[0] % 16) / sizeof(double);
    for (bx = 0; bx < L->num_my_boxes; bx++) base[bx] = B->pair_scratch + pad + (size_t)bx * 2 * (size_t)L->box_volume;
    HIP_OK(hpgmg_hip_memcpy_h2d(B->d_pair_base, base, (size_t)L->num_my_boxes * sizeof(double *)));
    free(base);
  }
}
void hpgmg_set_fused_sweeps(int on) { hp_switch_set(SW_FUSED_SWEEPS, on ? 1 : 0); }
void hpgmg_set_pair_min_cells(long long cells) { hp_switch_set(SW_PAIR_MIN_CELLS, cells > 0 ? cells : 2000000); }
/* common part: does the level qualify for the sweep-pair kernel, and are its two private vectors there?
 * The CPU oracle's fp32 mode (its fp32_pair_smooth) restates which smooth() calls read the fp32 coefficient copies, from the
 * level's geometry; keep the two in step.  With precision 32 on one rank they are exactly these:
 *   Chebyshev smoother, 4 sweeps, 7-point operator (VC or CC); Dirichlet boundary; x_id and rhs_id both not VECTOR_TEMP;
 *   dim.i * dim.j * dim.k >= HPGMG_PAIR_MIN_CELLS (default 2 000 000, hpgmg_set_pair_min_cells);
 *   dim.i % 128 == 0; box side a multiple of 128, or 128 % box side == 0 with box side >= 16; at most 1024 boxes (kPairMaxBoxes);
 *   boxes lexicographic and all on this rank (across ranks the coefficient streams stay fp64);
 *   HPGMG_FUSED_SWEEPS and HPGMG_GHOST_FREE at their defaults (on); the storage conditions of pair_supported_dims (16-byte aligned boxes at
 *   a constant distance) hold for every level the host layer creates. */
static int pair_kernel_ready(level_type *L, int x_id, int rhs_id, int sweeps) {
  hpgmg_config cfg;
  hpgmg_get_config(&cfg);
  backend_t *B = hp_backend_of(L);
  if (!hp_switch(SW_FUSED_SWEEPS) || sweeps != 4 || cfg.op != HPGMG_OP_7PT || !hp_ghost_free_mode() || stencil_get_shape() != STENCIL_SHAPE_STAR) return 0;
  if (L->boundary_condition.type != BC_DIRICHLET || x_id == VECTOR_TEMP || rhs_id == VECTOR_TEMP) return 0;
  if (B->all_faces_local) { if (!hpgmg_hip_smooth_cheby_pair_supported(&B->dev, hp_variant()) || !hp_boxes_lexicographic(L)) return 0; }
  else if (!hp_pair_halo_ready(L, B)) return 0;          /* faces owned by other ranks: two-deep halo, one exchange per pair */
  { /* the pass structure pays down to the 128^3 level of config 2 (2 M cells) since the kernel library picks the launch shape per launch: 36-46 us per pair of
     * sweeps there against 2 x 25 for the tiled single sweeps (with 16 waves per workgroup whatever the level it lost: 80 us) */
    if ((long long)L->dim.i * L->dim.j * L->dim.k < hp_switch(SW_PAIR_MIN_CELLS)) return 0;
  }
  hp_ensure_pair_scratch(L, B);
  hpgmg_hip_set_ghost_free(1);
  return 1;
}

/* ---- one sweep-pair launch.  (scr, id): vector `id` of the level (scr 0) or private vector `id` (scr 1).  Chebyshev: x0, xm1 -> out1 (x1), out2 (x2).
 * GSRB: x0 -> out2, colours `sweep` and `sweep + 1`; private vector `edge` is clobbered. */
typedef struct { int scr, id; } pair_vec;
typedef struct {
  level_type *L; backend_t *B;
  int gsrb, rhs_id;
  double a, b, h2inv;
  const float *const *c32;                        /* Chebyshev: the fp32 coefficient copies, or NULL */
  pair_vec x0, xm1, out1, out2;
  double c1a, c2a, c1b, c2b;                      /* Chebyshev: the coefficients of the two sweeps */
  int edge, sweep;                                /* GSRB */
  int discard_x1;                                 /* one-shot request: out1 is scratch to the caller, need not be stored */
  const hpgmg_hip_level *fold_Lc; int fold_id;    /* one-shot request: x0 is read as x0 + its coarse parent (vector fold_id of fold_Lc); NULL: as stored, or already requested by the caller */
} pair_launch;
/* the one-shot requests are consumed per launch, and a two-part launch is two launches: every one of them is made again before each part */
static int pair_issue(const pair_launch *p) {
  backend_t *B = p->B;
  const int v = hp_variant(), form_dinv = dinv_formable(B, p->a, p->b, p->h2inv);
  if (p->fold_Lc) hpgmg_hip_pair_fold_interpolation(p->fold_Lc, p->fold_id, 1.0);
  if (form_dinv && !p->gsrb && alpha_uniform_usable(B)) hpgmg_hip_pair_uniform_alpha(B->alpha_value);      /* one-shot like the others: made again before each part */
  if (p->gsrb) return hpgmg_hip_smooth_gsrb_pair(&B->dev, v, (double *const *)B->d_pair_base, NULL, p->x0.scr, p->x0.id, p->edge, p->out2.scr, p->out2.id, p->rhs_id, p->a, p->b, p->h2inv, p->sweep, form_dinv);
  return hpgmg_hip_smooth_cheby_pair(&B->dev, v, (double *const *)B->d_pair_base, p->c32, p->x0.scr, p->x0.id, p->xm1.scr, p->xm1.id, p->out1.scr, p->out1.id, p->out2.scr, p->out2.id,
                                     p->rhs_id, p->a, p->b, p->h2inv, p->c1a, p->c2a, p->c1b, p->c2b, form_dinv);
}
static void pair_part(const pair_launch *p, int remote, int part) {
  if (remote) { const pair_halo *H = p->B->halo; hpgmg_hip_pair_set_halo(H->brick, H->rem, H->deep, H->deep_beta); }
  if (part) hpgmg_hip_set_tile_part(part);
  if (p->discard_x1) hpgmg_hip_pair_discard_x1();
  HIP_OK(pair_issue(p));
}
/* local; remote: faces on other ranks, from the two-deep halo; remote and overlapped (hp_pair_halo_begin returned 1): the part that reads no halo under the exchange, then the rest */
static void pair_go(const pair_launch *p, int remote, int overlapped, const char *what) {
  level_type *L = p->L;
  TICK(L, smooth, what);
  if (overlapped) { pair_part(p, 1, 1); hp_overlap_end(); pair_part(p, 1, 2); hpgmg_hip_set_tile_part(0); }
  else pair_part(p, remote, 0);
  TOCK();
}

/* Chebyshev smooth() as fused sweep pairs (kernels/cheby_pair.hpp): 4 sweeps = 2 passes of 10 streams instead of
 * 4 x 9.  x1,x2 of the first pair go to two plugin-private vectors, the second pair brings x3 -> VECTOR_TEMP and
 * x4 -> x_id, i.e. exactly the state chebyshev.c:43-99 leaves.  Returns 0 when the level does not qualify. */
/* temp_dead: smooth() called by the cycle driver through hpgmg_smooth_in_cycle(): VECTOR_TEMP (x3 of the four sweeps) is dead after it, so the second
 * pair does not store it */
/* fold_Lc: interpolation_vcycle(L, x_id, 1.0, fold_Lc, x_id) is folded into the first pair (hp_interp_smooth_fused).  One rank: the caller has already told the
 * kernel library (hpgmg_hip_pair_fold_interpolation, consumed by the first pair launch).  Faces on other ranks: every owner adds the parents of the cells it
 * SENDS while packing the pair's halo, and the kernel adds them inside the brick only -- requested here, once per part of the two-part launch. */
static long long interp_folded_remote = 0;
long long hpgmg_interp_folded_remote(void) { return interp_folded_remote; }      /* smooth() calls across rank boundaries whose interpolation was folded in (tests) */
int hp_smooth_cheby_pairs(level_type *L, int x_id, int rhs_id, double a, double b, const double *c1, const double *c2, int sweeps, int temp_dead, const hpgmg_hip_level *fold_Lc) {
  if (!pair_kernel_ready(L, x_id, rhs_id, sweeps)) return 0;
  backend_t *B = hp_backend_of(L);
  const int remote = !B->all_faces_local;
  const float *const *c32 = remote ? NULL : coef32_of(L);      /* across ranks the coefficient streams stay fp64 */
  const pair_vec x = { 0, x_id }, temp = { 0, VECTOR_TEMP }, p0 = { 1, 0 }, p1 = { 1, 1 };
  pair_launch p = { .L = L, .B = B, .rhs_id = rhs_id, .a = a, .b = b, .h2inv = 1.0 / (L->h * L->h), .c32 = c32 };
  int over = 0;
  if (c32) fp32_pair_smooths++;
  if (remote) {
    pair_remote_smooths++;
    if (fold_Lc) { hpgmg_hip_pair_halo_fold_interpolation(fold_Lc, x_id, 1.0); interp_folded_remote++; p.fold_Lc = fold_Lc; p.fold_id = x_id; }
    over = hp_pair_halo_begin(L, B, 1, 0, x_id, 0, VECTOR_TEMP, rhs_id);
  }
  p.x0 = x; p.xm1 = temp; p.out1 = p0; p.out2 = p1; p.c1a = c1[0]; p.c2a = c2[0]; p.c1b = c1[1]; p.c2b = c2[1];
  pair_go(&p, remote, over, "smooth (Chebyshev sweeps 1+2)");
  if (remote) over = hp_pair_halo_begin(L, B, 0, 1, 1, 1, 0, rhs_id);
  p.x0 = p1; p.xm1 = p0; p.out1 = temp; p.out2 = x; p.c1a = c1[2]; p.c2a = c2[2]; p.c1b = c1[3]; p.c2b = c2[3];
  p.discard_x1 = temp_dead; p.fold_Lc = NULL;
  pair_go(&p, remote, over, "smooth (Chebyshev sweeps 3+4)");
  return 1;
}
/* in-place GSRB smooth() (gsrb.c:24-132, 4 coloured half sweeps) as two passes of two half sweeps each:
 * x_id -> private vector -> x_id; VECTOR_TEMP is not touched, as in the reference's in-place form */
int hp_smooth_gsrb_pairs(level_type *L, int x_id, int rhs_id, double a, double b, int sweeps) {
  if (hpgmg_gsrb_out_of_place() || !pair_kernel_ready(L, x_id, rhs_id, sweeps)) return 0;
  backend_t *B = hp_backend_of(L);
  const int remote = !B->all_faces_local;
  const pair_vec x = { 0, x_id }, p1 = { 1, 1 };
  pair_launch p = { .L = L, .B = B, .gsrb = 1, .rhs_id = rhs_id, .a = a, .b = b, .h2inv = 1.0 / (L->h * L->h), .edge = 0 };
  int over = 0;
  if (remote) { pair_remote_smooths++; over = hp_pair_halo_begin(L, B, 1, 0, x_id, 0, x_id, rhs_id); }
  p.x0 = x; p.out2 = p1; p.sweep = 0;
  pair_go(&p, remote, over, "smooth (GSRB half sweeps 1+2)");
  if (remote) over = hp_pair_halo_begin(L, B, 0, 1, 1, 1, 1, rhs_id);
  p.x0 = p1; p.out2 = x; p.sweep = 2;
  pair_go(&p, remote, over, "smooth (GSRB half sweeps 3+4)");
  return 1;
}

/* interpolation_vcycle(Lf, e, 1.0, Lc, e) followed by smooth(Lf, e, R) -- the up-leg of MGVCycle (mg.c:1160-1161) -- with the
 * piecewise-constant interpolation folded into the first sweep pair: the interpolated e is never written or re-read.
 * Same iterate (e = x4) as the two separate operators; VECTOR_TEMP (their x3) is left unspecified -- nothing in a cycle reads it
 * (HPGMG_TEMP_SCRATCH=0 stores it as smooth() does).  0 = not applicable. */
int hpgmg_interp_smooth_fused(level_type *Lf, int e_id, int R_id, level_type *Lc, double a, double b) { hp_lazy_flush(); return hp_interp_smooth_fused(Lf, e_id, R_id, Lc, a, b, 0); }
/* exact_state: VECTOR_TEMP is left as smooth() leaves it (the lazy queue runs behind the reference's own driver, which promises nothing about it) */
/* The same fold on the levels the sweep-pair kernel does not take (the cache-resident 128^3 ... 32^3 levels of config 2: single Chebyshev sweeps): sweep 0
 * reads x_n and sweep 1 reads x_{n-1} as stored + the coarse value above the cell (kernels/stencil_direct.hpp: InterpFold), so interpolation_vcycle is no
 * launch of its own.  The same iterates; the interpolated vector itself never exists, and VECTOR_TEMP ends as smooth() leaves it (x3). */
static long long interp_folded_single = 0;
long long hpgmg_interp_folded_single(void) { return interp_folded_single; }      /* (tests) */
static int interp_smooth_fused_single(level_type *Lf, int e_id, int R_id, level_type *Lc, double a, double b) {
  hpgmg_config cfg;
  hpgmg_get_config(&cfg);
  const int sweeps = hpgmg_smooth_sweeps(), v = hp_variant();
  communicator_type *S = &Lc->interpolation, *Rv = &Lf->interpolation;
  if (!hp_switch(SW_FUSED_RESIDUAL) || cfg.op != HPGMG_OP_7PT || cfg.smoother != HPGMG_SMOOTH_CHEBY || !Lf->active || !Lc->active || sweeps < 2) return 0;
  if (Lf->num_my_boxes < 1 || Lc->num_my_boxes < 1 || !hp_ghost_free_mode() || Lf->boundary_condition.type != BC_DIRICHLET) return 0;
  if (S->num_sends || Rv->num_recvs || S->num_blocks[0] || Rv->num_blocks[2]) return 0;   /* all parents local (the coarse level's send side, the fine level's receive side; their other sides belong to other level pairs) */
  if (e_id == VECTOR_TEMP || R_id == VECTOR_TEMP || Lf->dominant_eigenvalue_of_DinvA <= 0.0) return 0;
  backend_t *B = hp_backend_of(Lf), *Bc = hp_backend_of(Lc);
  if (!B->all_faces_local || stencil_get_shape() != STENCIL_SHAPE_STAR) return 0;
  hpgmg_hip_set_ghost_free(1);
  if (!hpgmg_hip_smooth_cheby_fold_supported(&B->dev, v)) return 0;
  const int *map = hp_restrict_map_of(Lf, B);
  if (!map) return 0;
  double c1[16], c2[16];
  const double h2inv = 1.0 / (Lf->h * Lf->h);
  int s;
  hp_cheby_coefficients(Lf, sweeps, c1, c2);
  B->img_active = 0;
  for (s = 0; s < sweeps; s++) {
    const int src = (s & 1) ? VECTOR_TEMP : e_id, dst = (s & 1) ? e_id : VECTOR_TEMP;
    TICK(Lf, smooth, s < 2 ? "smooth (Chebyshev sweep, interpolation folded in)" : "smooth");
    if (s < 2) hpgmg_hip_stencil_fold_interpolation(&Bc->dev, e_id, map, s + 1);
    HIP_OK(hpgmg_hip_smooth_cheby(&B->dev, v, src, dst, R_id, a, b, h2inv, c1[s], c2[s]));
    TOCK();
  }
  interp_folded_single++;
  return 1;
}
int hp_interp_smooth_fused(level_type *Lf, int e_id, int R_id, level_type *Lc, double a, double b, int exact_state) {
  hpgmg_config cfg;
  hpgmg_get_config(&cfg);
  const int sweeps = hpgmg_smooth_sweeps();
  communicator_type *S = &Lc->interpolation, *Rv = &Lf->interpolation;
  if (cfg.op != HPGMG_OP_7PT || !Lf->active || !Lc->active) return 0;
  if (cfg.smoother != HPGMG_SMOOTH_CHEBY && !(cfg.smoother == HPGMG_SMOOTH_GSRB && !hpgmg_gsrb_out_of_place())) return 0;
  if (S->num_sends || Rv->num_recvs || S->num_blocks[0] || Rv->num_blocks[2]) return 0;   /* all parents local (the coarse level's send side, the fine level's receive side; their other sides belong to other level pairs) */
  const int remote = !hp_backend_of(Lf)->all_faces_local;      /* across ranks: Chebyshev pairs only (every owner adds the parents to the halo cells it sends) */
  int parents_in_place = (Lc->num_my_boxes == Lf->num_my_boxes), bx;      /* the kernel finds the parent of a cell of fine box b in coarse box b */
  for (bx = 0; parents_in_place && bx < Lf->num_my_boxes; bx++)
    parents_in_place = (2 * Lc->my_boxes[bx].low.i == Lf->my_boxes[bx].low.i && 2 * Lc->my_boxes[bx].low.j == Lf->my_boxes[bx].low.j && 2 * Lc->my_boxes[bx].low.k == Lf->my_boxes[bx].low.k);
  if ((remote && Lf->box_dim % 128 != 0) || Lc->box_dim * 2 != Lf->box_dim || !parents_in_place ||      /* (narrow boxes across ranks: the fold stays with the single sweeps) */ (!remote && !hp_boxes_lexicographic(Lc)) ||
      (remote && (cfg.smoother != HPGMG_SMOOTH_CHEBY || !hp_switch(SW_PAIR_REMOTE))) ||
      !pair_kernel_ready(Lf, e_id, R_id, sweeps))
    return interp_smooth_fused_single(Lf, e_id, R_id, Lc, a, b);      /* (VECTOR_TEMP ends as smooth() leaves it: also for the queue) not a sweep-pair level: the fold of the single sweeps, if it is one of those */
  if (cfg.smoother == HPGMG_SMOOTH_CHEBY && Lf->dominant_eigenvalue_of_DinvA <= 0.0) return 0;
  if (!remote) hpgmg_hip_pair_fold_interpolation(&hp_backend_of(Lc)->dev, e_id, 1.0);
  if (cfg.smoother == HPGMG_SMOOTH_CHEBY) {
    double c1[16], c2[16];
    hp_cheby_coefficients(Lf, sweeps, c1, c2);
    const int done = hp_smooth_cheby_pairs(Lf, e_id, R_id, a, b, c1, c2, sweeps, !exact_state && hp_switch(SW_TEMP_SCRATCH), remote ? &hp_backend_of(Lc)->dev : NULL);      /* the cycle hook: VECTOR_TEMP is dead afterwards */
    if (!done) { fprintf(stderr, "hpgmg: fused interpolation+smooth refused after being accepted\n"); abort(); }
  } else if (!hp_smooth_gsrb_pairs(Lf, e_id, R_id, a, b, sweeps)) { fprintf(stderr, "hpgmg: fused interpolation+smooth refused after being accepted\n"); abort(); }
  return 1;
}
