/*
 * plugin_legs.c -- the fused legs of a cycle: a chain of small levels as one launch (the 7-point tail, the one-box tail of the other plugins), the launch-bound levels above it as brick visits, the device bottom solve.
 * Part of the operator plugin (see operators_hip.c); no arithmetic on vector data happens here.
 */
#include "plugin_internal.h"

/* fold the iteration counts of device-side bottom solves into level->Krylov_iterations (mg.c:156 prints it) */
void hpgmg_level_sync_counters(level_type *L) {
  hpgmg_hip_timer_flush();                       /* pending device timers land in level->timers before they are read or reset */
  hpgmg_level_ext *X = hpgmg_level_ext_get(L);
  backend_t *B = (backend_t *)X->backend;
  if (!B || !B->krylov_pinned) return;
  HIP_OK(hpgmg_hip_sync());
  L->Krylov_iterations += *B->krylov_pinned;
  *B->krylov_pinned = 0;
}

/* what a tail launch is told about the levels above it */
typedef struct {
  level_type *books_on;      /* the level whose timers take the tail launch when bricks were visited above it (NULL: the chain's own first level) */
  int follows_bricks;        /* the chain is what is left below levels visited as bricks */
} tail_ctx;
enum { TAIL_DOWN = 1, TAIL_BOTTOM = 2, TAIL_UP = 4, TAIL_WHOLE = 7 };      /* hpgmg_hip_small_tail_args.legs */

/* A V-cycle over a chain of tiny levels of the 27-point / fv2 / fv4 plugins (smooth ... bottom solve ... smooth as one launch): every level of the chain is ONE
 * box whose vectors fit the LDS (kernels/small_levels.hip: small_vtail_kernel).  `7 8`: the levels of 8^3, 4^3, 2^3 (and 1^3) cells. */
/* On by default except for the 27-point plugin with GSRB (HPGMG_SMALL_VTAIL=0 / 1, hpgmg_set_small_vtail(); bit-identical, tested both ways).
 * Measured on MI355X, `7 8` F-cycles with it on / off: fv4 GSRB 7.72 / 7.77 ms, fv4 Chebyshev 8.13 / 8.23, fv2 GSRB 6.35 / 6.56, fv2 Chebyshev
 * 6.65 / 6.91, 27-point Chebyshev 4.72 / 4.84 -- and 27-point GSRB 4.04 / 3.94: that plugin's one-launch red + black box kernel beats two half
 * sweeps of the generic form.  The first version (1024 lanes) was slower everywhere: the bottom solve's 240 registers per lane spilled into
 * scratch memory under the 128-register cap; with 512 lanes the launch of 8^3 + 4^3 + 2^3 levels takes 169 instead of 191 us (fv4 GSRB;
 * tools/exp_vtail_timeline.py): 4 x 24 us of smoothing, 28 us of bottom solve, the rest image traffic and interpolation. */
static long long small_vtails = 0;
long long hpgmg_small_vtails(void) { return small_vtails; }
void hpgmg_set_small_vtail(int on) { hp_switch_set(SW_SMALL_VTAIL, (on == 2) ? 2 : (on ? 1 : 0)); }      /* 0 off, 1 on for every plugin, 2 the default (not for 27-point GSRB) */
static int small_vtail_fused(level_type **levels, int n, int e_id, int R_id, double a, double b, int legs, int ask_only, const tail_ctx *ctx) {
  hpgmg_config cfg;
  hpgmg_hip_small_tail_args T;
  int l;
  const int small_vtail_on = (int)hp_switch(SW_SMALL_VTAIL);      /* 2: the default */
  if (!small_vtail_on) return 0;
  hpgmg_get_config(&cfg);
  if (small_vtail_on == 2 && cfg.op == HPGMG_OP_27PT && cfg.smoother == HPGMG_SMOOTH_GSRB && !ctx->follows_bricks) return 0;      /* (below brick launches it is the tail: the legs must stay whole) */
  const int sweeps = hpgmg_smooth_sweeps();
  if (n < 2 || n > HPGMG_HIP_SMALL_TAIL_MAX_LEVELS || sweeps < 1 || sweeps > 8 || (sweeps & 1) || hp_switch(SW_GRAPH)) return 0;      /* (captured segments: the argument block's upload is not capturable) */
  if (cfg.smoother != HPGMG_SMOOTH_CHEBY && cfg.smoother != HPGMG_SMOOTH_GSRB && cfg.smoother != HPGMG_SMOOTH_JACOBI) return 0;
  memset(&T, 0, sizeof T);
  T.n = n; T.legs = legs; T.mode = (cfg.smoother == HPGMG_SMOOTH_CHEBY) ? 0 : (cfg.smoother == HPGMG_SMOOTH_GSRB ? 1 : 2);
  T.sweeps = sweeps; T.out_of_place = (T.mode == 1) ? hpgmg_gsrb_out_of_place() : 0;
  T.e_id = e_id; T.R_id = R_id; T.krylov_base = hpgmg_vectors_reserved(); T.a = a; T.b = b; T.want = MG_DEFAULT_BOTTOM_NORM;
  const int shape = stencil_get_shape();
  for (l = 0; l < n; l++) {
    level_type *L = levels[l];
    if (!L->active || L->num_my_boxes != 1 || L->boxes_in.i * L->boxes_in.j * L->boxes_in.k != 1) return 0;
    if (L->boundary_condition.type != BC_DIRICHLET || L->dim.i != L->dim.j || L->dim.i != L->dim.k) return 0;
    if (l > 0 && 2 * L->dim.i != levels[l - 1]->dim.i) return 0;
    if (!hp_comm_nothing_to_exchange(&L->exchange_ghosts[shape]) || !hp_comm_nothing_to_exchange(&L->exchange_ghosts[STENCIL_SHAPE_BOX])) return 0;
    backend_t *B = hp_backend_of(L);
    hpgmg_hip_small_tail_level *v = &T.lv[l];
    v->L = B->dev;
    v->h2inv = 1.0 / (L->h * L->h);
    v->n_bc = L->boundary_condition.num_blocks[shape];
    v->bc_list = v->n_bc ? hp_mirror(L, L->boundary_condition.blocks[shape], v->n_bc) : NULL;
    const hp_small_bc bc = hp_small_bc_rule(cfg.op, L);
    v->bc_kind = bc.kind; v->zero_first = bc.zero_first;
    /* the conditions interpolation_vcycle applies to THIS level's correction before the level above reads it: apply_BCs_p2 (27-point) /
     * apply_BCs_v2 (fv2, fv4) over STENCIL_SHAPE_BOX */
    v->n_ibc = L->boundary_condition.num_blocks[STENCIL_SHAPE_BOX];
    v->ibc_list = v->n_ibc ? hp_mirror(L, L->boundary_condition.blocks[STENCIL_SHAPE_BOX], v->n_ibc) : NULL;
    const hp_small_bc ibc = hp_small_bc_rule(cfg.op == HPGMG_OP_FV4 ? HPGMG_OP_FV2 : cfg.op, L);
    v->ibc_kind = ibc.kind; v->ibc_zero_first = ibc.zero_first;
    if (v->n_bc > 32 || v->n_ibc > 32) return 0;
    if (l + 1 < n) {
      if (T.mode == 0) { if (L->dominant_eigenvalue_of_DinvA <= 0.0) return 0; hp_cheby_coefficients(L, sweeps, v->c1, v->c2); }
      if (T.mode == 2) { int q; for (q = 0; q < sweeps; q++) v->c2[q] = 2.0 / 3.0; }
    } else if (legs & TAIL_BOTTOM) {
      /* solvers.c:77-87: the fused solve is the Dirichlet one (no mean to remove); the Krylov vectors must exist */
      if (L->must_subtract_mean != 0) return 0;
      if ((long long)L->dim.i * L->dim.j * L->dim.k > hpgmg_hip_bottom_bicgstab_max_cells()) return 0;
      if (L->numVectors < hpgmg_vectors_reserved() + IterativeSolver_NumVectors()) return 0;
      T.krylov_iterations = hp_krylov_pinned(B);
      if (!T.krylov_iterations) return 0;
    }
  }
  if (hpgmg_hip_small_vtail_lds_doubles(&T) > hpgmg_hip_small_vtail_lds_limit()) return 0;
  if (ask_only) return 1;
  TICK(ctx->books_on ? ctx->books_on : levels[0], smooth, "fused V-cycle tail (levels of one box)");
  HIP_OK(hpgmg_hip_small_vtail(&T, hp_variant()));
  TOCK();
  small_vtails++;
  return 1;
}
void hpgmg_set_fused_tail(int on) { hp_switch_set(SW_FUSED_TAIL, on ? 1 : 0); }      /* tests: 0 = every operator of the small levels as its own launch(es) */
void hpgmg_set_fused_bottom(int on) { hp_switch_set(SW_FUSED_BOTTOM, on ? 1 : 0); }  /* tests: 0 = the bottom solve driven from the host (host/solvers.c BiCGStab through the operators) */
void hpgmg_set_brick_visits(int on) { hp_switch_set(SW_BRICK_VISITS, on ? 1 : 0); if (on == 8 || on == 16) hp_switch_set(SW_BRICK_SIZE, on); }      /* 0 off, 1 on, 8 / 16: on with bricks of that side */
long long hpgmg_brick_visits(void) { return hpgmg_hip_brick_visits(); }
void hpgmg_set_brick_wide(int on) { hp_switch_set(SW_BRICK_WIDE, on ? 1 : 0); }      /* 0: the 27-point / fv4 plugins visit their launch-bound levels launch by launch (tests) */
void hpgmg_set_brick_chains(int on) { hp_switch_set(SW_BRICK_CHAIN, on ? 1 : 0); }      /* 0: one launch per level visit instead of one per V-cycle leg (tests) */
/* what the kernels that address cells by global coordinate need of a level (tail.hip, brick_visit.hip): a cubic Dirichlet domain whose boxes are all
 * here, all faces local, local box b at lexicographic position b */
static int dense_level_ok(level_type *L) {
  backend_t *B = hp_backend_of(L);
  if (!L->active || L->num_my_boxes < 1 || !B->all_faces_local) return 0;
  if (L->boundary_condition.type != BC_DIRICHLET || L->dim.i != L->dim.j || L->dim.i != L->dim.k) return 0;
  return hp_boxes_lexicographic(L);
}
/* How many leading levels of the chain are visited as bricks of 8^3 / 16^3 cells, one launch per visit (kernels/brick_visit.hip): the levels of 64^3 / 32^3
 * cells above the single-workgroup tail.  0: none. */
static int brick_op_is_wide(const hpgmg_config *cfg) { return cfg->op == HPGMG_OP_27PT || cfg->op == HPGMG_OP_FV4; }
static long long brick_capacity_refusals = 0;
long long hpgmg_brick_capacity_refusals(void) { return brick_capacity_refusals; }      /* level visits left to the launch-by-launch path because the device does not hold that many bricks at once (tests) */
static int brick_prefix(level_type **levels, int n, const hpgmg_config *cfg) {
  const int sweeps = hpgmg_smooth_sweeps();
  int k = 0;
  const int wide = brick_op_is_wide(cfg);      /* 27-point / fv4: kernels/brick_wide.hip (bricks of 8^3 only, Chebyshev or out-of-place GSRB) */
  if (!hp_switch(SW_BRICK_VISITS) || !hp_switch(SW_FUSED_TAIL) || hp_switch(SW_GRAPH)) return 0;
  if (wide ? (!hp_switch(SW_BRICK_WIDE) || (cfg->smoother != HPGMG_SMOOTH_CHEBY && cfg->smoother != HPGMG_SMOOTH_GSRB) || (cfg->smoother == HPGMG_SMOOTH_GSRB && !hpgmg_gsrb_out_of_place()))
           : (!hp_ghost_free_mode() || cfg->op != HPGMG_OP_7PT)) return 0;
  if (sweeps < 1 || sweeps > hpgmg_hip_brick_visit_max_sweeps() || (sweeps & 1)) return 0;
  while (k + 1 < n) {
    level_type *L = levels[k];
    /* where the single-workgroup tail takes over: the 7-point tail holds levels up to 16^3; the tail of the other plugins starts at the first level of ONE box */
    const int fits_tail = wide ? (L->num_my_boxes == 1 && L->boxes_in.i * L->boxes_in.j * L->boxes_in.k == 1 && L->dim.i <= (int)hp_switch(SW_BRICK_WIDE_TAIL_DIM))
                               : ((long long)L->dim.i * L->dim.j * L->dim.k <= hpgmg_hip_tail_max_cells());
    if ((wide || L->dim.i < (int)hp_switch(SW_BRICK_MIN_DIM)) && fits_tail) break;
    if (wide && L->dim.i > (int)hp_switch(SW_BRICK_WIDE_MAX_DIM)) return 0;      /* (a tuning switch: all three launch-bound levels pay, profiles/r06d_ab_wide_max.txt) */
    if (!dense_level_ok(L) || !dense_level_ok(levels[k + 1]) || 2 * levels[k + 1]->dim.i != L->dim.i) return 0;
    const int wide_brick = wide ? hpgmg_hip_brick_wide_supported(&hp_backend_of(L)->dev, hp_variant()) : 0;      /* 8, 4 (the level of 4^3 cells) or 0 */
    if (wide ? !wide_brick
             : !hpgmg_hip_brick_visit_supported(&hp_backend_of(L)->dev, (int)hp_switch(SW_BRICK_SIZE))) { if (fits_tail) break; return 0; }
    { /* every brick of a launch must be running at once: more bricks than the device holds of this kernel = the launch-by-launch path (kernels/brick_visit.hip) */
      const int brick = wide ? wide_brick : (int)hp_switch(SW_BRICK_SIZE), side = L->dim.i / brick;
      const int capacity = wide ? hpgmg_hip_brick_wide_capacity(hp_variant(), cfg->smoother) : hpgmg_hip_brick_chain_capacity(hp_variant(), cfg->smoother, brick);
      if (side * side * side > capacity) { brick_capacity_refusals++; if (fits_tail) break; return 0; }
    }
    if (L->dominant_eigenvalue_of_DinvA <= 0.0 && cfg->smoother == HPGMG_SMOOTH_CHEBY) return 0;
    k++;
  }
  return k;
}
/* One launch of bricks for levels[first .. first + count - 1] (dir 0 down, 1 up, 2 interpolation_fcycle + down), or one per level when chains are off.
 * `top`: the level whose timers take the launches -- the one whose V-cycle this is, like the tail below it (mg.c books the whole fused cycle on that level's Total) */
static void brick_chain(level_type *top, level_type **levels, int first, int count, const hpgmg_config *cfg, int e_id, int R_id, double a, double b, int dir, int top_e_zero, int below_zero) {
  const int sweeps = hpgmg_smooth_sweeps(), chain = (int)hp_switch(SW_BRICK_CHAIN), max_n = (chain == 1 || (chain == 2 && dir != 1) || (chain == 3 && dir == 1)) ? hpgmg_hip_brick_chain_max_levels() : 1;
  int done = 0;
  while (done < count) {
    hpgmg_hip_brick_level lv[4];
    int n = count - done, j, s;
    if (n > max_n) n = max_n;
    if (brick_op_is_wide(cfg)) {
      /* the levels of one launch are cut into bricks of one size: the level of 4^3 cells (one brick of 4^3) goes on its own */
      const int v = hp_variant();
      if (dir == 1) { const int b0 = hpgmg_hip_brick_wide_supported(&hp_backend_of(levels[first + count - done - 1])->dev, v);
                      int m = 1; while (m < n && hpgmg_hip_brick_wide_supported(&hp_backend_of(levels[first + count - done - 1 - m])->dev, v) == b0) m++; n = m; }
      else          { const int b0 = hpgmg_hip_brick_wide_supported(&hp_backend_of(levels[first + done])->dev, v);
                      int m = 1; while (m < n && hpgmg_hip_brick_wide_supported(&hp_backend_of(levels[first + done + m])->dev, v) == b0) m++; n = m; }
    }
    /* down: the finest levels first; up: the coarsest levels first */
    const int lo = (dir == 1) ? first + count - done - n : first + done;
    for (j = 0; j < n; j++) {
      level_type *L = levels[lo + j];
      lv[j].L = hp_backend_of(L)->dev; lv[j].h2inv = 1.0 / (L->h * L->h);
      for (s = 0; s < 8; s++) lv[j].c1[s] = lv[j].c2[s] = 0.0;
      if (cfg->smoother == HPGMG_SMOOTH_CHEBY) hp_cheby_coefficients(L, sweeps, lv[j].c1, lv[j].c2);
    }
    const int is_first_launch = (done == 0), is_last_launch = (done + n == count);
    TICK(top, smooth, dir == 1 ? "level visits, up (bricks: interpolation + smooth per level, one launch)" :
                      (dir == 0 ? "level visits, down (bricks: smooth + residual + restriction per level, one launch)" : "interpolation_fcycle + level visit, down (bricks, one launch)"));
    if (brick_op_is_wide(cfg))
      HIP_OK(hpgmg_hip_brick_wide_chain(n, lv, &hp_backend_of(levels[lo + n])->dev, sweeps, hp_variant(), cfg->smoother, e_id, R_id, a, b, dir,
                                        dir == 0 ? (is_first_launch ? top_e_zero : 1) : 0, (dir != 1 && is_last_launch) ? below_zero : 0));
    else
    HIP_OK(hpgmg_hip_brick_chain(n, lv, &hp_backend_of(levels[lo + n])->dev, sweeps, hp_variant(), cfg->smoother, e_id, R_id, a, b, dir, (int)hp_switch(SW_BRICK_SIZE),
                                 dir == 0 ? (is_first_launch ? top_e_zero : 1) : 0, (dir != 1 && is_last_launch) ? below_zero : 0));
    TOCK();
    done += n;
  }
}

/* IterativeSolver's BiCGStab on a bottom level of one small box of the 27-point / fv2 / fv4 plugins as ONE launch (kernels/small_levels.hip:
 * bottom_bicgstab_kernel; the 7-point plugin's bottom solve lives in its tail kernel).  Driven from the host, an iteration is ~25 launches and
 * ~6 host round trips on a level of 8 cells.  HPGMG_FUSED_BOTTOM=0 keeps the host-driven solver. */
static int bottom_solve_fused_impl(level_type *L, int e_id, int R_id, double a, double b, double want, int ask_only) {
  hpgmg_config cfg;
  const int on = (int)hp_switch(SW_FUSED_BOTTOM);
  hpgmg_get_config(&cfg);
  if (!on || cfg.op == HPGMG_OP_7PT || !L->active || L->num_my_boxes != 1 || L->boxes_in.i * L->boxes_in.j * L->boxes_in.k != 1) return 0;
  if (e_id >= hpgmg_vectors_reserved() || R_id >= hpgmg_vectors_reserved()) return 0;       /* they alias the host solver's work vectors (tail_legs) */
  if (L->boundary_condition.type == BC_PERIODIC || L->must_subtract_mean == 1) return 0;
  if ((long long)L->dim.i * L->dim.j * L->dim.k > hpgmg_hip_bottom_bicgstab_max_cells()) return 0;
  const int shape = stencil_get_shape();
  if (!hp_comm_nothing_to_exchange(&L->exchange_ghosts[shape])) return 0;
  const int n_bc = L->boundary_condition.num_blocks[shape];
  const hp_small_bc bc = hp_small_bc_rule(cfg.op, L);
  if (L->numVectors < hpgmg_vectors_reserved() + IterativeSolver_NumVectors()) return 0;      /* (the solver's work vectors must exist) */
  if (ask_only) return 1;
  hp_lazy_flush();
  backend_t *B = hp_backend_of(L);
  if (!hp_krylov_pinned(B)) return 0;
  /* no tick of its own: the caller (MGVCycle -> IterativeSolver) already charges the bottom solve to L->timers.Total */
  HIP_OK(hpgmg_hip_bottom_bicgstab(&B->dev, hp_variant(), e_id, R_id, hpgmg_vectors_reserved(), a, b, 1.0 / (L->h * L->h), want,
                                   n_bc ? hp_mirror(L, L->boundary_condition.blocks[shape], n_bc) : NULL, n_bc, bc.kind, bc.zero_first, B->krylov_pinned));
  return 1;
}
int hpgmg_bottom_solve_fused(level_type *L, int e_id, int R_id, double a, double b, double want) { return bottom_solve_fused_impl(L, e_id, R_id, a, b, want, 0); }

/* The tail forms of a leg over levels[0 .. n-1], each one launch: what is left of the 27-point / fv2 / fv4 V-cycle below bricks, their one-box tail, and
 * the 7-point tail (kernels/tail.hip: both legs of a V-cycle over a chain of tiny levels, with or without the bottom solve).
 * probe: would the leg be taken?  (nothing is launched) */
static int tail_legs(level_type **levels, int n, const hpgmg_config *cfg, int e_id, int R_id, double a, double b, int leg, int probe, const tail_ctx *ctx) {
  const hpgmg_hip_level *dev[8];
  int l, s;
  double h2inv[8], c1[64], c2[64];
  const int enabled = (int)hp_switch(SW_FUSED_TAIL), bottom_enabled = (int)hp_switch(SW_FUSED_BOTTOM);
  const int with_bottom = (leg != HPGMG_LEG_DOWN && leg != HPGMG_LEG_UP), ftail = (leg == HPGMG_LEG_FCYCLE_TAIL || leg == HPGMG_LEG_FCYCLE_TAIL_ASK);
  /* A correction or right-hand side that lives among the work vectors of the host-driven Krylov solver (ids >= VECTORS_RESERVED: MGPCG's z,
   * mg.c:1530) ALIASES them on the bottom level -- z is BiCGStab's p there (solvers/bicgstab.c:14-19) -- and the reference's numbers include that.
   * The fused bottom solve keeps the solver's vectors to itself, so the forms that contain it step aside: the legs run without it and the host-driven
   * solver goes through the operators, aliasing included. */
  if (with_bottom && (e_id >= hpgmg_vectors_reserved() || R_id >= hpgmg_vectors_reserved())) return 0;
  if (with_bottom && hpgmg_get_bottom_solver() != HPGMG_BOTTOM_BICGSTAB) return 0;        /* the device bottom solve is BiCGStab: another host solver runs through the operators */
  const int sweeps = hpgmg_smooth_sweeps();
  if (enabled && cfg->op != HPGMG_OP_7PT && n == 1 && ctx->follows_bricks && leg <= HPGMG_LEG_VCYCLE) {
    /* every level above the bottom one was visited as bricks: what is left of the V-cycle is the bottom solve or nothing (the legs around a host-driven one) */
    if (leg != HPGMG_LEG_VCYCLE) return 1;
    return bottom_enabled ? bottom_solve_fused_impl(levels[0], e_id, R_id, a, b, MG_DEFAULT_BOTTOM_NORM, probe) : 0;
  }
  if (enabled && cfg->op != HPGMG_OP_7PT) {      /* DOWN / UP: the way down / up around a bottom solve somebody else runs (the reference's driver, through the queue) */
    if (leg == HPGMG_LEG_VCYCLE) return bottom_enabled ? small_vtail_fused(levels, n, e_id, R_id, a, b, TAIL_WHOLE, probe, ctx) : 0;
    if (leg == HPGMG_LEG_DOWN || leg == HPGMG_LEG_UP) return small_vtail_fused(levels, n, e_id, R_id, a, b, leg == HPGMG_LEG_DOWN ? TAIL_DOWN : TAIL_UP, probe, ctx);
    return 0;
  }
  if (!enabled || !hp_ghost_free_mode() || cfg->op != HPGMG_OP_7PT || n > 8 || n > hpgmg_hip_tail_max_levels() || sweeps > 8) return 0;
  if (with_bottom && !bottom_enabled) return 0;
  if (n < (leg == HPGMG_LEG_BOTTOM ? 1 : 2)) return 0;
  if (ftail && (!hp_switch(SW_FUSED_FTAIL) || levels[0]->dim.i > (int)hp_switch(SW_FTAIL_MAX_DIM))) return 0;
  /* multi-rank jobs: the chain qualifies when this rank owns every box of every level in it (dense_level_ok), which is
   * how the coarse levels end up after agglomeration onto rank 0 -- no message and no all-reduce is needed then */
  for (l = 0; l < n; l++) {
    level_type *L = levels[l];
    const long long cells = (long long)L->dim.i * L->dim.j * L->dim.k;
    /* the kernel addresses cells by global coordinate: cubic Dirichlet domain, boxes in lexicographic order, halving per level */
    if (!dense_level_ok(L) || (sweeps & 1)) return 0;
    if (l > 0 && 2 * L->dim.i != levels[l - 1]->dim.i) return 0;
    backend_t *B = hp_backend_of(L);
    if (l + 1 < n) {
      if (cells > hpgmg_hip_tail_max_cells()) return 0;
      if (L->dominant_eigenvalue_of_DinvA <= 0.0 && cfg->smoother == HPGMG_SMOOTH_CHEBY) return 0;
      hp_cheby_coefficients(L, sweeps, c1 + l * sweeps, c2 + l * sweeps);
    } else {
      for (s = 0; s < sweeps; s++) c1[l * sweeps + s] = c2[l * sweeps + s] = 0.0;
      if (with_bottom) {
        /* solvers.c:27-95: Dirichlet never subtracts the mean; the Krylov vectors must exist */
        if (cells > hpgmg_hip_tail_bottom_max_cells() || L->must_subtract_mean == 1) return 0;
        if (L->numVectors < hpgmg_vectors_reserved() + IterativeSolver_NumVectors()) return 0;
        L->must_subtract_mean = 0;
        if (!hp_krylov_pinned(B)) return 0;
      }
    }
    dev[l] = &B->dev;
    h2inv[l] = 1.0 / (L->h * L->h);
  }
  if (leg == HPGMG_LEG_FCYCLE_TAIL_ASK || probe) return 1;
  TICK(ctx->books_on ? ctx->books_on : levels[0], smooth, leg == HPGMG_LEG_BOTTOM ? "bottom solve (device BiCGStab)" : (leg == HPGMG_LEG_FCYCLE_TAIL ? "fused F-cycle tail" : "fused V-cycle tail"));
  HIP_OK(hpgmg_hip_vcycle_tail(n, dev, h2inv, c1, c2, sweeps, hp_variant(), cfg->smoother, e_id, R_id, a, b, leg,
                               hpgmg_vectors_reserved(), MG_DEFAULT_BOTTOM_NORM, with_bottom ? hp_backend_of(levels[n - 1])->krylov_pinned : NULL));
  TOCK();
  return 1;
}
/* `leg`: enum hpgmg_leg (include/hpgmg_operators.h), + HPGMG_LEG_ASK: only answer */
int hp_vcycle_legs_fused(level_type **levels, int n, int e_id, int R_id, double a, double b, int leg) {
  hpgmg_config cfg;
  const tail_ctx whole = { NULL, 0 };
  const int probe = (leg >= HPGMG_LEG_ASK);
  hpgmg_get_config(&cfg);
  if (probe) leg -= HPGMG_LEG_ASK;
  if ((leg <= HPGMG_LEG_VCYCLE || leg == HPGMG_LEG_FCYCLE_STEP) && !probe) {
    /* launch-bound levels above the tail: one launch per level visit, then the tail, then one launch per visit on the way up.  FCYCLE_STEP: the step of
     * FMGSolve's climb (mg.c:1289-1293): interpolation_fcycle(levels[0] <- levels[1]) rides in the first launch of the V-cycle that follows it --
     * every brick of that launch reads levels[1]'s correction, so its zero_vector is left to the launch that visits levels[1] (a brick level too). */
    const int fstep = (leg == HPGMG_LEG_FCYCLE_STEP), vleg = fstep ? HPGMG_LEG_VCYCLE : leg;
    if (fstep && (!hp_switch(SW_BRICK_FSTEP) || brick_op_is_wide(&cfg))) return 0;      /* (27-point / fv4: interpolation_fcycle stays a launch of its own) */
    const int k = brick_prefix(levels, n, &cfg);
    const tail_ctx below = { levels[0], 1 };
    if (k > (fstep ? 1 : 0) && tail_legs(levels + k, n - k, &cfg, e_id, R_id, a, b, vleg, 1, &below)) {
      /* zero_vector of a brick level below the first: by the launch that visits it (which then does not read the vector either); the tail's first level: here */
      if (vleg != HPGMG_LEG_UP) {
        if (fstep) { brick_chain(levels[0], levels, 0, 1, &cfg, e_id, R_id, a, b, 2, 0, 0); brick_chain(levels[0], levels, 1, k - 1, &cfg, e_id, R_id, a, b, 0, 1, 1); }
        else brick_chain(levels[0], levels, 0, k, &cfg, e_id, R_id, a, b, 0, 0, 1);
      }
      if (!tail_legs(levels + k, n - k, &cfg, e_id, R_id, a, b, vleg, 0, &below)) { fprintf(stderr, "hpgmg: the V-cycle tail was refused after being accepted\n"); abort(); }
      if (vleg != HPGMG_LEG_DOWN) brick_chain(levels[0], levels, 0, k, &cfg, e_id, R_id, a, b, 1, 0, 0);
      return 1;
    }
  }
  if (leg == HPGMG_LEG_FCYCLE_STEP) return 0;
  return tail_legs(levels, n, &cfg, e_id, R_id, a, b, leg, probe, &whole);
}
int hpgmg_vcycle_legs_fused(level_type **levels, int n, int e_id, int R_id, double a, double b, int leg) { hp_lazy_flush(); return hp_vcycle_legs_fused(levels, n, e_id, R_id, a, b, leg); }
