/*
 * plugin_smooth.c -- smooth() (operators/chebyshev.c, gsrb.c, jacobi.c) as the dispatcher of its forms: single sweeps, red + black passes, one small level as one launch (the sweep pairs: plugin_pairs.c; the fused legs: plugin_legs.c); residual() / apply_op().
 * Part of the operator plugin (see operators_hip.c); no arithmetic on vector data happens here.
 */
#include "plugin_internal.h"

/* ---------------------------------------------------------------- smoothers */
void hp_cheby_coefficients(const level_type *L, int degree, double *c1, double *c2) { /* chebyshev.c:22-40 */
  double beta = 1.000 * L->dominant_eigenvalue_of_DinvA, alpha = 0.125000 * beta;
  double theta = 0.5 * (beta + alpha), delta = 0.5 * (beta - alpha), sigma = theta / delta, rho_n = 1 / sigma;
  int s;
  c1[0] = 0.0; c2[0] = 1 / theta;
  for (s = 1; s < degree; s++) { double rho_nm1 = rho_n; rho_n = 1.0 / (2.0 * sigma - rho_nm1); c1[s] = rho_n * rho_nm1; c2[s] = rho_n * 2.0 / delta; }
}

/* Small levels of the 27-point / fv2 / fv4 plugins: smooth(), residual() or apply_op() with their exchange_boundary + apply_BCs steps as
 * ONE single-workgroup launch (kernels/small_levels.hip: small_level_kernel).
 * Returns 0 when the level does not qualify (too large, messages needed, 7-point plugin: that one has the LDS-resident tail kernel).
 * OFF by default (HPGMG_SMALL_FUSED=1 enables; bit-identical, covered by the GPU tests): measured on MI355X it is SLOWER than the
 * launches it replaces -- fv4 GSRB `7 8` 17.1 vs 12.7 ms, 27-pt GSRB 9.9 vs 6.2 ms per F-cycle -- because a 16^3 level in 8 boxes has
 * ~160 copy / boundary list entries whose dependent load chains run 16 at a time on one CU, while separate launches spread them over
 * the chip; the launch overhead saved (~5 us each) is smaller than that serialisation. */
void hpgmg_set_small_fused(int mode) { hp_switch_set(SW_SMALL_FUSED, (mode == 1 || mode == 2) ? 2 : 0); }   /* 0 off, 1 every small level, 2 (default) one-box levels in LDS */
enum { SMALL_CHEBY = 0, SMALL_GSRB = 1, SMALL_JACOBI = 2, SMALL_RESIDUAL = 3, SMALL_APPLY_OP = 4 };      /* hpgmg_hip_small_level_op's mode */
static int small_level_try(level_type *L, int mode, int x_id, int rhs_id, int res_id, double a, double b) {
  hpgmg_config cfg;
  const int small_fused = hp_switch(SW_SMALL_FUSED) ? 2 : 0;      /* (mode 1, every small level out of global memory, measured slower in two rounds: removed) */
  /* 0: off.  1 (experiment builds): every qualifying level, out of global memory (slower than the launches it replaces, see above).  2
   * (default): smooth() on levels of ONE box whose vectors fit the LDS -- the kernel then works on an image of the box there (round 3).  With
   * generic (FLAT) accesses to the image a smooth() was one ~60 us launch instead of twelve ~5 us ones: no gain.  With LDS-typed pointers, the
   * boundary descriptors built without scratch memory and the corner / edge extrapolations of apply_BCs_v4 spread over the lanes of a wave it
   * is 27 us (fv4, 8^3): `7 8` fv4 9.45 -> 9.2 ms, fv2 7.05 -> 6.45 ms per F-cycle.  Bit-identical, tested in all three modes. */
  hpgmg_get_config(&cfg);
  /* mode 2 takes what it shortens: a smooth() of many launches (fv4 GSRB: 12, Chebyshev: 8; a residual or apply_op is two launches of ~5 us,
   * the kernel with its copies in and out ~15 us; the 27-point GSRB smoother already runs as two one-workgroup-per-box launches) */
  const int small_27 = (int)hp_switch(SW_SMALL_27PT_GSRB);
  const int smoother = (mode <= SMALL_JACOBI);
  const int worth = smoother && (small_27 || !(cfg.op == HPGMG_OP_27PT && cfg.smoother == HPGMG_SMOOTH_GSRB));
  const int enabled = (small_fused == 2 && worth && L->num_my_boxes == 1 && (size_t)9 * (size_t)L->box_volume * sizeof(double) <= (size_t)150 * 1024);
  if (!enabled || cfg.op == HPGMG_OP_7PT || L->num_my_boxes < 1) return 0;
  if ((long long)L->dim.i * L->dim.j * L->dim.k > hpgmg_hip_small_level_max_cells()) return 0;
  if (L->num_my_boxes != L->boxes_in.i * L->boxes_in.j * L->boxes_in.k) return 0;
  const int shape = stencil_get_shape();
  communicator_type *C = &L->exchange_ghosts[shape];
  if (!hp_comm_no_messages(C)) return 0;      /* (the kernel is handed the copies between local boxes) */
  hp_small_bc bc = { 0, 0 };
  int n_bc = 0;
  if (L->boundary_condition.type != BC_PERIODIC) { n_bc = L->boundary_condition.num_blocks[shape]; bc = hp_small_bc_rule(cfg.op, L); }
  const int sweeps = smoother ? hpgmg_smooth_sweeps() : 1;
  double c1[16], c2[16];
  int q;
  for (q = 0; q < 16; q++) c1[q] = c2[q] = 0.0;
  if (mode == SMALL_CHEBY) hp_cheby_coefficients(L, sweeps, c1, c2);
  if (mode == SMALL_JACOBI) for (q = 0; q < sweeps; q++) c2[q] = 2.0 / 3.0;
  if (sweeps > 8) return 0;
  backend_t *B = hp_backend_of(L);
  const double t_h2inv = 1.0 / (L->h * L->h);
  hpgmg_tick tk = hpgmg_tick_begin(L, smoother ? &L->timers.smooth : (mode == SMALL_RESIDUAL ? &L->timers.residual : &L->timers.apply_op), "small level, one launch");
  HIP_OK(hpgmg_hip_small_level_op(&B->dev, hp_variant(), mode, sweeps, x_id, rhs_id, res_id, mode == SMALL_GSRB ? hpgmg_gsrb_out_of_place() : 0, a, b, t_h2inv, c1, c2,
                                  hp_mirror(L, C->blocks[1], C->num_blocks[1]), C->num_blocks[1],
                                  n_bc ? hp_mirror(L, L->boundary_condition.blocks[shape], n_bc) : NULL, n_bc, bc.kind, bc.zero_first));
  hpgmg_tick_end(tk);
  return 1;
}

/* smooth() as the cycle driver uses it (mg.c:1148,1161): same iterate, but VECTOR_TEMP is left unspecified -- the next operator of a
 * cycle overwrites or ignores it.  Always returns 1 (the hook exists so that the reference's own driver, which never calls it, keeps
 * the exact state of smooth()). */
int hpgmg_smooth_in_cycle(level_type *L, int x_id, int rhs_id, double a, double b) {
  hp_lazy_flush();
  hp_do_smooth(L, x_id, rhs_id, a, b, (int)hp_switch(SW_TEMP_SCRATCH));
  return 1;
}
/* 4th-order operator, GSRB, inside a cycle (VECTOR_TEMP is scratch afterwards): each red + black pair of half sweeps as ONE pass
 * (kernels/fv4_rb.hpp) instead of gsrb.c:24-132's two.  The passes go x -> TEMP -> private vector 0 -> x (an odd number of passes cannot
 * ping-pong between two vectors); private vector 1 lends its k ghost planes to the intermediate vector's boundary values (the pre-pass).
 * 0 = not applicable, the caller runs the half sweeps one by one. */
static long long fv4_rb_smooths = 0, rb27_smooth_passes = 0;
long long hpgmg_rb27_passes(void) { return rb27_smooth_passes; }      /* red + black passes of the 27-point GSRB smoother so far (tests) */
long long hpgmg_fv4_rb_smooths(void) { return fv4_rb_smooths; }
static void fv4_rb_bcs(level_type *L, backend_t *B, int scratch, int id) {           /* apply_BCs_v4 on the pass's input (neighbouring boxes are read where they live) */
  const int shape = stencil_get_shape();
  if (L->boundary_condition.type == BC_PERIODIC) return;
  if (!scratch) { if (!hp_exchange_and_bcs_one_launch(L, id, shape, 4, 0)) apply_BCs(L, id, shape); return; }
  int n = 0;
  const hpgmg_hip_bc_entry *e = hp_bc_entries(L, shape, &n);
  hpgmg_hip_level Ls = B->dev;
  Ls.box_base = (double *const *)B->d_pair_base;
  TICK(L, boundary_conditions, "apply_BCs_v4 (private vector)");
  HIP_OK(hpgmg_hip_exchange_and_bc(&Ls, id, NULL, 0, e, n, 4));
  TOCK();
}
/* The cells whose intermediate value the one-pass kernel must not recompute: a cell next to a tile of ANOTHER box (= on an internal box face) whose
 * stencil reaches outside the domain (= within one cell of a wall in another direction).  The coefficient ghost cells outside the domain are
 * extrapolated with box-relative normals (boundary_fv.c:573-681), so two boxes hold different values for the same place there. */
static const int *fv4_special_cells(level_type *L, backend_t *B, int *n_out) {
  if (B->n_fv4_special < 0) {
    int cap = 1024, n = 0, b, ax, side, u, v;
    int *h = (int *)malloc((size_t)cap * 4 * sizeof(int));
    const int dim = L->box_dim, N[3] = { L->dim.i, L->dim.j, L->dim.k }, nb[3] = { L->boxes_in.i, L->boxes_in.j, L->boxes_in.k };
    if (L->boundary_condition.type != BC_PERIODIC)
    for (b = 0; b < L->num_my_boxes; b++) {
      const int low[3] = { L->my_boxes[b].low.i, L->my_boxes[b].low.j, L->my_boxes[b].low.k };
      for (ax = 0; ax < 3; ax++) for (side = 0; side < 2; side++) {
        const int bpos = low[ax] / dim + (side ? 1 : -1);
        if (bpos < 0 || bpos >= nb[ax]) continue;                          /* a domain wall, not an internal face */
        const int a1 = (ax + 1) % 3, a2 = (ax + 2) % 3;
        for (v = 0; v < dim; v++) for (u = 0; u < dim; u++) {
          const int g1 = low[a1] + u, g2 = low[a2] + v;
          if (!(g1 == 0 || g1 == N[a1] - 1 || g2 == 0 || g2 == N[a2] - 1)) continue;
          int c[3];
          c[ax] = side ? dim - 1 : 0; c[a1] = u; c[a2] = v;
          if (n == cap) { cap *= 2; h = (int *)realloc(h, (size_t)cap * 4 * sizeof(int)); }
          h[4 * n] = b; h[4 * n + 1] = c[0]; h[4 * n + 2] = c[1]; h[4 * n + 3] = c[2]; n++;
        }
      }
    }
    B->d_fv4_special = (int *)hpgmg_hip_malloc((size_t)(n > 0 ? n : 1) * 4 * sizeof(int));
    if (!B->d_fv4_special) { fprintf(stderr, "hpgmg: device allocation failed: %s\n", hpgmg_hip_last_error()); abort(); }
    if (n > 0) HIP_OK(hpgmg_hip_memcpy_h2d(B->d_fv4_special, h, (size_t)n * 4 * sizeof(int)));
    free(h);
    B->n_fv4_special = n;
  }
  *n_out = B->n_fv4_special;
  return B->d_fv4_special;
}
static int smooth_fv4_rb(level_type *L, int x_id, int rhs_id, double a, double b, int sweeps, int temp_dead) {
  hpgmg_config cfg;
  hpgmg_get_config(&cfg);
  backend_t *B = hp_backend_of(L);
  const int passes = sweeps / 2, v = hp_variant();
  if (cfg.op != HPGMG_OP_FV4 || !hpgmg_gsrb_out_of_place() || !temp_dead || !hp_ghost_free_mode() || (sweeps & 1) || passes < 1) return 0;
  if (L->num_my_boxes < 1 || x_id == VECTOR_TEMP || rhs_id == VECTOR_TEMP || L->box_dim < 8) return 0;
  /* boxes on other ranks: the same passes on the table with their images (halo_images.c) -- x three cells deep once per PASS, i.e. one
   * exchange per sweep where the reference has two (gsrb.c:30-33), the cells next to the faces recomputed from the owner's inputs */
  const int images = !B->all_faces_local;
  if (images && !hp_images_ready(L, B)) return 0;
  const hpgmg_hip_level *dev = images ? &B->img->dev : &B->dev;
  if (!hpgmg_hip_smooth_gsrb_fv4_rb_supported(dev, v)) return 0;
  int n_k = 0, k_local = 1, n_all = 0, p;
  const hpgmg_hip_bc_entry *e_k = NULL;
  if (images) e_k = hp_images_bc_k(L, B, &n_k);
  else if (L->boundary_condition.type != BC_PERIODIC) {
    e_k = hp_bc_entries_k(L, &n_k, &k_local);
    (void)hp_bc_entries(L, stencil_get_shape(), &n_all);
    if (!k_local || !B->bc_sources_local[stencil_get_shape()]) return 0;
  }
  hp_ensure_pair_scratch(L, B);
  double *const *pair_base = images ? (double *const *)B->img->d_pair_base : (double *const *)B->d_pair_base;
  hpgmg_hip_set_tile_ghost_free(1);
  const double h2inv = 1.0 / (L->h * L->h);
  int n_sp = 0;
  const int *sp_cells = images ? hp_images_fv4_special(L, B, &n_sp) : fv4_special_cells(L, B, &n_sp);
  /* (scratch, id) of the iterate before pass p: x, then TEMP / x alternately; an odd count routes its second pass through private vector 0 */
  int src_s = 0, src_id = x_id;
  for (p = 0; p < passes; p++) {
    int dst_s = 0, dst_id;
    const int left = passes - p;                   /* passes still to do, this one included */
    if (left == 1) dst_id = (passes == 1) ? VECTOR_TEMP : x_id;
    else if (left == 2 && !(src_s == 0 && src_id == x_id)) { dst_s = 1; dst_id = 0; }    /* two to go and not standing on x: step aside so that the last pass can land on x */
    else dst_id = (src_s == 0 && src_id == VECTOR_TEMP) ? x_id : VECTOR_TEMP;
    if (left == 2 && src_s == 0 && src_id == x_id) dst_id = VECTOR_TEMP;
    /* images: the message and the images' boundary conditions go to the exchange stream; under them the launch stream runs the tiles that
     * read neither an image nor anything the pre-pass forms (part 1), then waits, runs the pre-pass and the other tiles (part 2) */
    int overlapped = 0;
    if (images) overlapped = hp_images_refresh_begin(L, B, src_s, src_id, 3, p == 0 ? rhs_id : -1, 4);
    else fv4_rb_bcs(L, B, src_s, src_id);
    TICK(L, smooth, "smooth (fv4 GSRB, red + black half sweeps in one pass)");
    /* the pre-pass also works on the images next to the k walls: the main kernel reads the intermediate vector's ghost planes in their columns */
    LAUNCH_IN_PARTS(overlapped, HIP_OK(hpgmg_hip_fv4_rb_prepass(images ? &B->img->dev_all : dev, v, pair_base, src_s, src_id, 1, rhs_id, a, b, h2inv, 2 * p, e_k, n_k, sp_cells, n_sp)),
                    hpgmg_hip_smooth_gsrb_fv4_rb(dev, v, pair_base, src_s, src_id, dst_s, dst_id, 1, rhs_id, a, b, h2inv, 2 * p));
    TOCK();
    src_s = dst_s; src_id = dst_id;
  }
  if (passes == 1) hp_do_scale_vector(L, x_id, 1.0, VECTOR_TEMP);      /* a single pass cannot land on its own input (never the case with the reference's counts) */
  fv4_rb_smooths++;
  return 1;
}
/* temp_dead: the caller declares VECTOR_TEMP scratch after this smooth() (inside a cycle: hpgmg_smooth_in_cycle, or the operator queue saw it
 * overwritten next) -- the in-cycle forms may run: the sweep pair without the x3 store, the red + black passes of the 27-point / fv4 GSRB smoothers */
void hp_do_smooth(level_type *L, int x_id, int rhs_id, double a, double b, int temp_dead) {
  hpgmg_config cfg;
  hpgmg_get_config(&cfg);
  const int sweeps = hpgmg_smooth_sweeps(), v = hp_variant();
  const double h2inv = 1.0 / (L->h * L->h);
  backend_t *B = hp_backend_of(L);
  int s;
  if (cfg.op != HPGMG_OP_7PT && small_level_try(L, cfg.smoother == HPGMG_SMOOTH_CHEBY ? SMALL_CHEBY : (cfg.smoother == HPGMG_SMOOTH_GSRB ? SMALL_GSRB : SMALL_JACOBI), x_id, rhs_id, x_id, a, b)) return;
  if (cfg.smoother == HPGMG_SMOOTH_CHEBY) {          /* chebyshev.c:8-100 */
    double c1[16], c2[16];
    if (L->dominant_eigenvalue_of_DinvA <= 0.0 && L->my_rank == 0) fprintf(stderr, "dominant_eigenvalue_of_DinvA <= 0.0 !\n");
    hp_cheby_coefficients(L, sweeps, c1, c2);
    if (hp_smooth_cheby_pairs(L, x_id, rhs_id, a, b, c1, c2, sweeps, temp_dead, NULL)) return;
    for (s = 0; s < sweeps; s++) {
      const int src = (s & 1) ? VECTOR_TEMP : x_id, dst = (s & 1) ? x_id : VECTOR_TEMP;
      STENCIL_WITH_GHOSTS(L, src, dst, smooth, hpgmg_hip_smooth_cheby(hp_stencil_dev(B), v, src, dst, rhs_id, a, b, h2inv, c1[s], c2[s]));
    }
  } else if (cfg.smoother == HPGMG_SMOOTH_GSRB) {    /* gsrb.c:24-132 */
    const int oop = hpgmg_gsrb_out_of_place();
    if (hp_smooth_gsrb_pairs(L, x_id, rhs_id, a, b, sweeps)) return;
    /* 27-point, inside a cycle (VECTOR_TEMP is scratch afterwards): each red + black pair of half sweeps as one pass, x -> TEMP -> x.
     * The state the exported smooth() must leave in VECTOR_TEMP (the iterate before the last half sweep) never exists in this form. */
    if (cfg.op == HPGMG_OP_27PT && oop && temp_dead && hp_ghost_free_mode() && sweeps % 4 == 0 && L->num_my_boxes > 0 &&
        (B->all_faces_local || hp_images_ready(L, B)) && x_id != VECTOR_TEMP && rhs_id != VECTOR_TEMP) {
      /* boxes on other ranks: the same pass on the table with their images -- x two cells deep once per pass (one exchange per sweep instead of
       * gsrb.c:30-33's two), the intermediate vector on the cells around a box recomputed from the owner's x, right-hand side and D^{-1} */
      const int images = !B->all_faces_local;
      const hpgmg_hip_level *dev = images ? &B->img->dev : &B->dev;
      const int tiled = hpgmg_hip_smooth_gsrb27_rb_supported(dev);                          /* boxes of side 64 m: marching tiles */
      const int boxed = !tiled && hpgmg_hip_smooth_gsrb27_rb_box_supported(dev);   /* boxes of 2^3 ... 16^3: one workgroup per box */
      if (tiled || boxed) {
        for (s = 0; s < sweeps; s += 2) {
          const int src = (s & 2) ? VECTOR_TEMP : x_id, dst = (s & 2) ? x_id : VECTOR_TEMP;
          int overlapped = 0;
          if (images && tiled) overlapped = hp_images_refresh_begin(L, B, 0, src, 2, s == 0 ? rhs_id : -1, 12);     /* the tiles that read no image run under the exchange */
          else if (images) hp_images_refresh(L, B, 0, src, 2, s == 0 ? rhs_id : -1, 12);
          else if (tiled && !hp_exchange_and_bcs_one_launch(L, src, stencil_get_shape(), 12, 0)) apply_BCs(L, src, stencil_get_shape());
          TICK(L, smooth, "smooth (27-point GSRB, red + black half sweeps in one pass)");
          if (tiled) LAUNCH_IN_PARTS(overlapped, (void)0, hpgmg_hip_smooth_gsrb27_rb(dev, src, dst, rhs_id, a, b, h2inv, s));      /* (overlapped: tiled, with images) */
          else       HIP_OK(hpgmg_hip_smooth_gsrb27_rb_box(dev, src, dst, rhs_id, a, b, h2inv, s));
          TOCK();
          rb27_smooth_passes++;
        }
        return;
      }
    }
    if (smooth_fv4_rb(L, x_id, rhs_id, a, b, sweeps, temp_dead)) return;
    /* The exported smooth() (VECTOR_TEMP must be left as the separate half sweeps leave it: the iterate before the last one) -- what the
     * reference's own driver calls (Route B): all sweeps but the last as red + black passes x -> TEMP -> x, the last sweep as its two half
     * sweeps x -> TEMP -> x.  The same iterates, the same final x and VECTOR_TEMP; 2 passes + 2 half sweeps instead of 6 half sweeps. */
    int first_half_sweep = 0;
    if (cfg.op == HPGMG_OP_FV4 && oop && !temp_dead && sweeps >= 6 && !(sweeps & 1) && (((sweeps - 2) / 2) & 1) == 0 && !hp_switch(SW_FV4_NO_EXACT_RB)) {
      if (smooth_fv4_rb(L, x_id, rhs_id, a, b, sweeps - 2, 1)) first_half_sweep = sweeps - 2;      /* VECTOR_TEMP is scratch to THESE passes (the half sweeps after them rewrite it); an even number of passes: they end on x */
    }
    for (s = first_half_sweep; s < sweeps; s++) {
      const int src = (oop && (s & 1)) ? VECTOR_TEMP : x_id, dst = oop ? ((s & 1) ? x_id : VECTOR_TEMP) : x_id;
      STENCIL_WITH_GHOSTS(L, src, dst, smooth, hpgmg_hip_smooth_gsrb(hp_stencil_dev(B), v, src, dst, rhs_id, a, b, h2inv, s));
    }
  } else {                                           /* jacobi.c:8-65 */
    for (s = 0; s < sweeps; s++) {
      const int src = (s & 1) ? VECTOR_TEMP : x_id, dst = (s & 1) ? x_id : VECTOR_TEMP;
      STENCIL_WITH_GHOSTS(L, src, dst, smooth, hpgmg_hip_smooth_jacobi(hp_stencil_dev(B), v, src, dst, rhs_id, a, b, h2inv, 2.0 / 3.0));
    }
  }
}

void hp_do_residual(level_type *L, int res_id, int x_id, int rhs_id, double a, double b) {   /* residual.c:9-51 */
  if (small_level_try(L, SMALL_RESIDUAL, x_id, rhs_id, res_id, a, b)) return;
  STENCIL_WITH_GHOSTS(L, x_id, res_id, residual, hpgmg_hip_residual(hp_stencil_dev(hp_backend_of(L)), hp_variant(), res_id, x_id, rhs_id, a, b, 1.0 / (L->h * L->h)));
}
void hp_do_apply_op(level_type *L, int Ax_id, int x_id, double a, double b) {               /* apply_op.c:9-48 */
  if (small_level_try(L, SMALL_APPLY_OP, x_id, -1, Ax_id, a, b)) return;
  STENCIL_WITH_GHOSTS(L, x_id, Ax_id, apply_op, hpgmg_hip_residual(hp_stencil_dev(hp_backend_of(L)), hp_variant(), Ax_id, x_id, -1, a, b, 1.0 / (L->h * L->h)));
}
