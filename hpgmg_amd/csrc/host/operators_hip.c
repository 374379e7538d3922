/*
 * operators_hip.c -- the product's operator plugin: implements every symbol of
 * include/hpgmg_operators.h (= reference finite-volume/source/operators.h:14-50)
 * by forwarding to the gfx950 kernels behind include/hpgmg_hip.h.
 *
 * It plays the role operators.7pt.c plays in the reference (it is the ONE
 * operators.X.c compiled into the binary), but contains no arithmetic on vector
 * data: vectors live in device memory, this file only sequences launches and
 * keeps device mirrors of the immutable block lists.  There is no CPU fallback:
 * if a kernel launch fails the process aborts with the HIP error.
 *
 * Host-side structure of each routine follows the reference routine named in
 * its comment (exchange -> BC -> kernel, pack -> send/recv -> local -> unpack).
 *
 * Since round 4 the plugin is several translation units around plugin_internal.h:
 *   operators_hip.c     (this file) restriction, interpolation, the fused residual passes, BLAS-1 and reductions
 *   plugin_runtime.c    timers, storage hooks, transports, the per-level device record
 *   plugin_ghosts.c     exchange_boundary, apply_BCs_*, the overlapped exchange, black-box rebuild
 *   plugin_smooth.c     smooth(), residual(), apply_op(): which form each takes; single sweeps, red + black passes, one small level as one launch
 *   plugin_pairs.c      smooth() as sweep pairs, the interpolation folded into them, the fp32 coefficient copies
 *   plugin_legs.c       the fused legs of a cycle: brick visits, the single-launch tails, the device bottom solve
 *   plugin_pair_halo.c  the two-deep halo of the sweep pairs across ranks
 *   halo_images.c       images of the neighbouring ranks' boxes (27-point / fv4 across ranks)
 *   plugin_problem.c    initialize_problem, rebuild_operator
 *   plugin_queue.c      the lazy operator queue + the exported operators that pass through it
 *   plugin_switches.c   the run-time switches, one table
 */
#include "plugin_internal.h"

/* ---------------------------------------------------------------- restriction.c:104-212 */
void hp_do_restriction(level_type *Lc, int id_c, level_type *Lf, int id_f, int type) {
  TICK(Lf, restriction_total, "restriction");
  hp_coef_written(Lc, id_c);                           /* (a restriction into a coefficient vector: VECTOR_DINV no longer follows from them) */
  communicator_type *S = &Lf->restriction[type], *R = &Lc->restriction[type];
  backend_t *Bc = hp_backend_of(Lc), *Bf = hp_backend_of(Lf);
  HIP_OK(hpgmg_hip_restrict_blocks(&Bc->dev, id_c, &Bf->dev, id_f, hp_mirror(Lf, S->blocks[0], S->num_blocks[0]), S->num_blocks[0], type));
  hp_transport_phase(R, S, (Lf->tag << 4) | 0x5);
  HIP_OK(hpgmg_hip_restrict_blocks(&Bc->dev, id_c, &Bf->dev, id_f, hp_mirror(Lf, S->blocks[1], S->num_blocks[1]), S->num_blocks[1], type));
  HIP_OK(hpgmg_hip_copy_blocks(&Bc->dev, id_c, hp_mirror(Lc, R->blocks[2], R->num_blocks[2]), R->num_blocks[2]));
  TOCK();
}

/* restriction(Lc, id_c, Lf, id_f, RESTRICT_CELL) followed by zero_vector(Lc, zero_id) -- the end of MGVCycle's down-leg
 * (mg.c:1152-1153) -- as one launch when every contribution is local.  0 = the driver calls the two operators. */
int hpgmg_restrict_zero_fused(level_type *Lc, int id_c, level_type *Lf, int id_f, int zero_id) {
  communicator_type *S = &Lf->restriction[RESTRICT_CELL], *R = &Lc->restriction[RESTRICT_CELL];
  if (!Lf->active || !Lc->active || Lc->num_my_boxes < 1 || zero_id == id_c) return 0;
  if (S->num_sends || R->num_recvs || S->num_blocks[0] || R->num_blocks[2] || S->num_blocks[1] < 1) return 0;
  TICK(Lf, restriction_total, "restriction + zero_vector");
  backend_t *Bc = hp_backend_of(Lc), *Bf = hp_backend_of(Lf);
  HIP_OK(hpgmg_hip_restrict_cell_and_zero(&Bc->dev, id_c, &Bf->dev, id_f, hp_mirror(Lf, S->blocks[1], S->num_blocks[1]), S->num_blocks[1], zero_id));
  TOCK();
  return 1;
}

/* residual(Lf, TEMP, x, rhs) ; restriction(Lc, id_c, Lf, TEMP, RESTRICT_CELL) ; zero_vector(Lc, zero_id) -- the end of MGVCycle's down
 * leg (mg.c:1150-1153) -- as ONE pass over the fine level: the residual is restricted on the fly and never stored (VECTOR_TEMP of the
 * fine level keeps its previous content; nothing reads it before the up leg's smooth() overwrites it).  0 = not applicable. */
/* per fine box: the coarse box it restricts into and the coarse cell under its first cell -- read off the local restriction list */
static const int *restrict_map_of(level_type *Lf, backend_t *Bf);
const int *hp_restrict_map_of(level_type *Lf, backend_t *Bf) { return restrict_map_of(Lf, Bf); }
static const int *restrict_map_of(level_type *Lf, backend_t *Bf) {
  communicator_type *S = &Lf->restriction[RESTRICT_CELL];
  if (!Bf->d_restrict_map) {
    int *map = (int *)malloc((size_t)Lf->num_my_boxes * 4 * sizeof(int)), n, b;
    for (b = 0; b < 4 * Lf->num_my_boxes; b++) map[b] = -1;
    for (n = 0; n < S->num_blocks[1]; n++) {
      const blockCopy_type *e = &S->blocks[1][n];
      if (e->read.box < 0 || e->write.box < 0 || map[4 * e->read.box] >= 0) continue;
      map[4 * e->read.box] = e->write.box;
      map[4 * e->read.box + 1] = e->write.i - e->read.i / 2; map[4 * e->read.box + 2] = e->write.j - e->read.j / 2; map[4 * e->read.box + 3] = e->write.k - e->read.k / 2;
    }
    for (b = 0; b < Lf->num_my_boxes; b++) if (map[4 * b] < 0) { free(map); return NULL; }
    Bf->d_restrict_map = (int *)hpgmg_hip_malloc((size_t)Lf->num_my_boxes * 4 * sizeof(int));
    if (!Bf->d_restrict_map) { fprintf(stderr, "hpgmg: device allocation failed: %s\n", hpgmg_hip_last_error()); abort(); }
    HIP_OK(hpgmg_hip_memcpy_h2d(Bf->d_restrict_map, map, (size_t)Lf->num_my_boxes * 4 * sizeof(int)));
    free(map);
  }
  return Bf->d_restrict_map;
}
static long long fused_residuals_remote = 0;
long long hpgmg_fused_residuals_remote(void) { return fused_residuals_remote; }      /* fused residual passes on levels with faces on other ranks, 7-point (tests) */
static int fused_residual_on(void) {
  return (int)hp_switch(SW_FUSED_RESIDUAL);
}
/* the operand of a fused residual form is made ready: 7-point -- nothing (the kernel applies the Dirichlet rule and reads neighbouring boxes);
 * 27-point / fv4 -- the domain-boundary ghost cells (the tiled kernel reads neighbouring boxes itself).  0 = the level does not qualify;
 * 2 = x is crossing faces to other ranks on the exchange stream: FUSED_LAUNCH issues the pass as the tiles that touch no such face, the wait, the others. */
/* B: the level of the pass.  Where its alpha is known to be uniform the launch is told so (one-shot, consumed by the launch: hp_alpha_uniform_arm_residual; one rank only) */
#define FUSED_LAUNCH(B, READY, CALL) do {                                                                       \
    if ((READY) == 2) {                                                                                          \
      hpgmg_hip_set_tile_part(1); HIP_OK(CALL); hp_overlap_end(); hpgmg_hip_set_tile_part(2); HIP_OK(CALL); hpgmg_hip_set_tile_part(0); \
    } else HIP_OK((hp_alpha_uniform_arm_residual(B), CALL));      /* (armed inside HIP_OK: behind the operators it issues first) */ \
  } while (0)
static int fused_residual_operand_form(level_type *L, backend_t *B, int x_id, int restrict_form);
static int fused_residual_operand(level_type *L, backend_t *B, int x_id) { return fused_residual_operand_form(L, B, x_id, 0); }
/* restrict_form: residual + restriction + zero_vector, which the 7-point plugin also has for the launch-bound levels of small boxes (one launch instead of two) */
static int fused_residual_operand_form(level_type *L, backend_t *B, int x_id, int restrict_form) {
  hpgmg_config cfg;
  hpgmg_get_config(&cfg);
  const int shape = stencil_get_shape();
  if (!fused_residual_on() || !hp_ghost_free_mode() || !L->active || L->num_my_boxes < 1 || L->boundary_condition.type == BC_PERIODIC) return 0;
  B->img_active = 0;
  if (!B->all_faces_local && cfg.op == HPGMG_OP_7PT) {
    /* 7-point with faces on other ranks: the kernel reads a remote face's neighbour from the ghost zone, so x crosses those faces first (one cell
     * deep, in stream order).  The pass saves 74 - 58 B per cell against residual + restriction; that pays for an exchange the separate residual()
     * would have hidden under its interior only on a bandwidth-bound level (the threshold of the sweep pairs) */
    if (shape != STENCIL_SHAPE_STAR || (long long)L->num_my_boxes * L->box_dim * L->box_dim * L->box_dim < hp_switch(SW_PAIR_MIN_CELLS)) return 0;
    hpgmg_hip_set_ghost_free(1);
    if (!hpgmg_hip_residual_fused_supported(&B->dev, hp_variant())) return 0;
    fused_residuals_remote++;
    if (hp_overlap_begin(L, x_id)) return 2;      /* the exchange runs on the second stream: the caller launches the pass in its two parts */
    hp_ghosts_for_stencil(L, x_id, -1);
    return 1;
  }
  if (!B->all_faces_local) {           /* 27-point / fv4 with boxes on other ranks: the same pass on the table with their images */
    if ((cfg.op != HPGMG_OP_27PT && cfg.op != HPGMG_OP_FV4) || !hp_images_ready(L, B) || !hpgmg_hip_residual_fused_supported(&B->img->dev, hp_variant())) return 0;
    hpgmg_hip_set_ghost_free(0);
    hpgmg_hip_set_tile_ghost_free(1);
    hp_images_refresh(L, B, 0, x_id, stencil_get_radius(), -1, cfg.op == HPGMG_OP_27PT ? 12 : 4);
    return 1;
  }
  if (cfg.op == HPGMG_OP_7PT) {
    if (shape != STENCIL_SHAPE_STAR) return 0;
    hpgmg_hip_set_ghost_free(1);
    return restrict_form ? hpgmg_hip_residual_restrict_supported(&B->dev, hp_variant()) : hpgmg_hip_residual_fused_supported(&B->dev, hp_variant());
  }
  if (cfg.op != HPGMG_OP_27PT && cfg.op != HPGMG_OP_FV4) return 0;
  if (!hpgmg_hip_residual_fused_supported(&B->dev, hp_variant())) return 0;
  hpgmg_hip_set_ghost_free(0);
  hpgmg_hip_set_tile_ghost_free(1);
  if (!hp_exchange_and_bcs_one_launch(L, x_id, shape, cfg.op == HPGMG_OP_27PT ? 12 : 4, 0)) apply_BCs(L, x_id, shape);
  return 1;
}
int hpgmg_residual_restrict_zero_fused(level_type *Lc, int id_c, level_type *Lf, int x_id, int rhs_id, double a, double b, int zero_id) {
  hp_lazy_flush();
  return hp_residual_restrict_zero_fused(Lc, id_c, Lf, -1, x_id, rhs_id, a, b, zero_id);
}
/* res_id >= 0: the residual is stored as well (7-point): the exact state of the three operators */
int hp_residual_restrict_zero_fused(level_type *Lc, int id_c, level_type *Lf, int res_id, int x_id, int rhs_id, double a, double b, int zero_id) {
  communicator_type *S = &Lf->restriction[RESTRICT_CELL], *R = &Lc->restriction[RESTRICT_CELL];
  if (!Lf->active || !Lc->active || Lc->num_my_boxes < 1 || Lf->num_my_boxes < 1 || zero_id == id_c) return 0;
  if (S->num_sends || R->num_recvs || S->num_blocks[0] || R->num_blocks[2] || S->num_blocks[1] < 1) return 0;
  backend_t *Bc = hp_backend_of(Lc), *Bf = hp_backend_of(Lf);
  if (!restrict_map_of(Lf, Bf)) return 0;
  { hpgmg_config cfg; hpgmg_get_config(&cfg); if (res_id >= 0 && (cfg.op != HPGMG_OP_7PT || res_id == x_id || res_id == rhs_id)) return 0; }
  const int ready = fused_residual_operand_form(Lf, Bf, x_id, 1);
  if (!ready) return 0;
  TICK(Lf, residual, "residual + restriction + zero_vector (fused)");
  FUSED_LAUNCH(Bf, ready, hpgmg_hip_residual_restrict_store(hp_stencil_dev(Bf), hp_variant(), res_id, x_id, rhs_id, a, b, 1.0 / (Lf->h * Lf->h), &Bc->dev, id_c, Bf->d_restrict_map, zero_id));
  TOCK();
  return 1;
}
/* norm(L, F) ; scale_vector(L, R, 1.0, F) ; restriction(Lc, R, L, R, RESTRICT_CELL) -- how FMGSolve starts (mg.c:1262-1270) -- in one pass over F.
 * Every rank's share of the restriction must be local.  0 = not applicable. */
int hp_norm_scale_restrict_fused(level_type *L, int F_id, int R_id, level_type *Lc, double *norm_out) {
  communicator_type *S = &L->restriction[RESTRICT_CELL], *R = &Lc->restriction[RESTRICT_CELL];
  if (!fused_residual_on() || !L->active || !Lc->active || L->num_my_boxes < 1 || Lc->num_my_boxes < 1 || F_id == R_id) return 0;
  if (S->num_sends || R->num_recvs || S->num_blocks[0] || R->num_blocks[2] || S->num_blocks[1] < 1) return 0;
  backend_t *Bc = hp_backend_of(Lc), *B = hp_backend_of(L);
  if ((L->box_dim & 1) || !(B->dev.flags & 1) || (L->box_jStride & 1) || (L->box_kStride & 1) || (L->box_volume & 1) || L->box_dim < 16) return 0;
  if (!restrict_map_of(L, B)) return 0;
  double v = 0.0;
  { TICK(L, blas1, norm_out ? "norm(F) + R = F + restriction (fused)" : "R = F + restriction (fused)");
    HIP_OK(hpgmg_hip_norm_copy_restrict(&B->dev, F_id, R_id, &Bc->dev, R_id, B->d_restrict_map, norm_out ? &v : NULL));
    TOCK(); }
  if (norm_out) *norm_out = hp_allreduce_scalar(L, v, HPGMG_REDUCE_MAX);
  return 1;
}
int hpgmg_norm_scale_restrict_fused(level_type *L, int F_id, int R_id, level_type *Lc, double *norm_out) { return hp_norm_scale_restrict_fused(L, F_id, R_id, Lc, norm_out); }
/* the same, the norm collected later by hpgmg_norm_deferred_fetch(L): FMGSolve needs norm(F) only for the convergence check at its end (mg.c:1262,1323), so the
 * host does not wait for this pass and keeps the stream full behind it */
static level_type *deferred_norm_level = NULL;
static double deferred_host_value = 0.0;
static int deferred_on_device = 0;
int hpgmg_norm_scale_restrict_fused_deferred(level_type *L, int F_id, int R_id, level_type *Lc) {
  communicator_type *S = &L->restriction[RESTRICT_CELL], *R = &Lc->restriction[RESTRICT_CELL];
  const hpgmg_transport *T = hpgmg_get_transport();
  const int many = (T && T->size > 1);
  if (!fused_residual_on() || !hp_switch(SW_DEFER_NORM) || !L->active || !Lc->active || F_id == R_id) return 0;
  /* Deferring moves a rank's reduction from the start of the solve to its end, so EVERY rank must take the same decision (a rank that reduced at the
   * start would pair its collective with another rank's at the end).  With several ranks the decision is therefore taken from what every rank knows:
   * the same box grid with the same owner for every box on both levels -- then the restriction is local on every rank. */
  if (many) {
    const int nb = L->boxes_in.i * L->boxes_in.j * L->boxes_in.k;
    int q;
    if (Lc->boxes_in.i != L->boxes_in.i || Lc->boxes_in.j != L->boxes_in.j || Lc->boxes_in.k != L->boxes_in.k) return 0;
    for (q = 0; q < nb; q++) if (L->rank_of_box[q] != Lc->rank_of_box[q]) return 0;
  }
  /* what THIS rank's one-pass kernel needs; a rank of a several-rank job that lacks it still defers: it issues the three operators and keeps its maximum */
  int local_ok = (L->num_my_boxes >= 1 && Lc->num_my_boxes >= 1 && !S->num_sends && !R->num_recvs && !S->num_blocks[0] && !R->num_blocks[2] && S->num_blocks[1] >= 1);
  backend_t *Bc = Lc->num_my_boxes >= 1 ? hp_backend_of(Lc) : NULL, *B = L->num_my_boxes >= 1 ? hp_backend_of(L) : NULL;
  if (local_ok && ((L->box_dim & 1) || !(B->dev.flags & 1) || (L->box_jStride & 1) || (L->box_kStride & 1) || (L->box_volume & 1) || L->box_dim < 16 || !restrict_map_of(L, B))) local_ok = 0;
  if (!local_ok && !many) return 0;
  if (local_ok) {
    TICK(L, blas1, "norm(F) + R = F + restriction (fused, norm deferred)");
    HIP_OK(hpgmg_hip_norm_copy_restrict_deferred(&B->dev, F_id, R_id, &Bc->dev, R_id, B->d_restrict_map));
    TOCK();
    deferred_on_device = 1;
  } else {
    double v = 0.0;
    if (B) { TICK(L, blas1, "norm(F), this rank's part (reduction deferred)"); HIP_OK(hpgmg_hip_norm_max(&B->dev, F_id, &v)); TOCK(); }
    hp_do_scale_vector(L, R_id, 1.0, F_id);
    hp_do_restriction(Lc, R_id, L, R_id, RESTRICT_CELL);
    deferred_host_value = v; deferred_on_device = 0;
  }
  deferred_norm_level = L;
  return 1;
}
double hpgmg_norm_deferred_fetch(level_type *L) {
  double v = deferred_host_value;
  if (deferred_norm_level != L) { fprintf(stderr, "hpgmg: no deferred norm is pending on this level\n"); abort(); }
  deferred_norm_level = NULL;
  if (deferred_on_device) HIP_OK(hpgmg_hip_deferred_fetch(&v));
  return hp_allreduce_scalar(L, v, HPGMG_REDUCE_MAX);
}
/* residual(L, res, x, rhs) ; norm(L, res) -- the convergence check of MGSolve / FMGSolve (mg.c:1321-1323) -- in one pass: the residual is
 * stored as usual (res_id < 0: not stored -- the cycle driver's check, after which VECTOR_TEMP is dead) and its max-abs comes out of the
 * same kernel.  0 = not applicable. */
int hpgmg_residual_norm_fused(level_type *L, int res_id, int x_id, int rhs_id, double a, double b, double *norm_out) {
  hpgmg_config cfg;
  hpgmg_get_config(&cfg);
  if (cfg.op != HPGMG_OP_7PT && res_id >= 0) return 0;          /* the tiled kernels of the other plugins only carry the norm-only form */
  if (!L->active || L->num_my_boxes < 1) return 0;
  backend_t *B = hp_backend_of(L);
  const int ready = fused_residual_operand(L, B, x_id);
  if (!ready) return 0;
  double v = 0.0;
  { TICK(L, residual, "residual + norm (fused)");
    FUSED_LAUNCH(B, ready, hpgmg_hip_residual_norm(hp_stencil_dev(B), hp_variant(), res_id, x_id, rhs_id, a, b, 1.0 / (L->h * L->h), &v));
    TOCK(); }
  *norm_out = hp_allreduce_scalar(L, v, HPGMG_REDUCE_MAX);
  return 1;
}

/* ---------------------------------------------------------------- interpolation_p0.c:52-159, interpolation_p1.c:70-180 */

static void interpolation_lists(level_type *Lf, int id_f, double prescale, level_type *Lc, int id_c, int order, int tagbits) {
  TICK(Lf, interpolation_total, "interpolation");
  hp_coef_written(Lf, id_f);
  communicator_type *S = &Lc->interpolation, *R = &Lf->interpolation;
  backend_t *Bc = hp_backend_of(Lc), *Bf = hp_backend_of(Lf);
  HIP_OK(hpgmg_hip_interpolate_blocks(&Bf->dev, id_f, 0.0, &Bc->dev, id_c, hp_mirror(Lc, S->blocks[0], S->num_blocks[0]), S->num_blocks[0], order));
  hp_transport_phase(R, S, (Lf->tag << 4) | tagbits);
  HIP_OK(hpgmg_hip_interpolate_blocks(&Bf->dev, id_f, prescale, &Bc->dev, id_c, hp_mirror(Lc, S->blocks[1], S->num_blocks[1]), S->num_blocks[1], order));
  HIP_OK(hpgmg_hip_increment_blocks(&Bf->dev, id_f, prescale, hp_mirror(Lf, R->blocks[2], R->num_blocks[2]), R->num_blocks[2]));
  TOCK();
}
void hp_do_interpolation_vcycle(level_type *Lf, int id_f, double prescale, level_type *Lc, int id_c) {
  hpgmg_config c; hpgmg_get_config(&c);
  if (c.op == HPGMG_OP_27PT) {                                  /* interpolation_p2.c:228-230 */
    if (!hp_exchange_and_bcs_one_launch(Lc, id_c, STENCIL_SHAPE_BOX, 12, 1)) { exchange_boundary(Lc, id_c, STENCIL_SHAPE_BOX); apply_BCs_p2(Lc, id_c, STENCIL_SHAPE_BOX); }
    interpolation_lists(Lf, id_f, prescale, Lc, id_c, 2, 0x7);
    return;
  }
  if (c.op == HPGMG_OP_FV2 || c.op == HPGMG_OP_FV4) {           /* interpolation_v2.c:210-212 (V-cycle of fv2 and fv4) */
    if (!hp_exchange_and_bcs_one_launch(Lc, id_c, STENCIL_SHAPE_BOX, 2, 1)) { exchange_boundary(Lc, id_c, STENCIL_SHAPE_BOX); apply_BCs_v2(Lc, id_c, STENCIL_SHAPE_BOX); }
    interpolation_lists(Lf, id_f, prescale, Lc, id_c, 3, 0x7);
    return;
  }
  if (c.op != HPGMG_OP_7PT) hp_no_kernel("interpolation_vcycle for this operator");
  interpolation_lists(Lf, id_f, prescale, Lc, id_c, 0, 0x6);
}
/* every parent of the fine level's cells is a local box-to-box entry (what the one-launch forms below need) */
static int interp_all_local(level_type *Lf, level_type *Lc) {
  communicator_type *S = &Lc->interpolation, *R = &Lf->interpolation;
  int n;
  if (Lc->num_my_boxes < 1 || S->num_sends || R->num_recvs || S->num_blocks[0] || R->num_blocks[2] || S->num_blocks[1] < 1) return 0;
  for (n = 0; n < S->num_blocks[1]; n++) if (S->blocks[1][n].read.box < 0 || S->blocks[1][n].write.box < 0) return 0;
  return 1;
}
/* zero_vector(Lf, id_f) ; interpolation_fcycle(Lf, id_f, 0.0, Lc, id_c) -- how the benchmark's step reaches the fine level: zero_vector(u) before
 * FMGSolve (hpgmg-fv.c:77-85), whose first write of u on that level is this interpolation (mg.c:1295) -- with the fine vector neither zeroed nor read
 * (0.0 * 0.0 + y): one pass over the fine level less.  7-point, ghost-free mode, every box local: the interior is exactly what the two operators leave;
 * the ghost zones, which zero_vector would clear, keep their content -- nothing reads them before a launch that needs them fills them.
 * 0 = the caller issues both. */
static long long zero_interp_fused = 0;
long long hpgmg_zero_interp_fused(void) { return zero_interp_fused; }
int hpgmg_zero_interpolation_fcycle_fused(level_type *Lf, int id_f, level_type *Lc, int id_c) {
  hpgmg_config c; hpgmg_get_config(&c);
  if (!hp_switch(SW_FUSED_RESIDUAL) || !hp_ghost_free_mode() || !Lf->active || !Lc->active || Lf->num_my_boxes < 1) return 0;
  if (!interp_all_local(Lf, Lc) || !hp_backend_of(Lf)->all_faces_local) return 0;
  zero_interp_fused++;
  /* the coarse operand's ghost zones as interpolation_fcycle() fills them, then the interpolation in its "onto zeros" form (order + 16) */
  if (c.op == HPGMG_OP_7PT) {                                   /* interpolation_p1.c:71-72 */
    if (!hp_exchange_and_bcs_one_launch(Lc, id_c, STENCIL_SHAPE_BOX, 1, 1)) { exchange_boundary(Lc, id_c, STENCIL_SHAPE_BOX); apply_BCs_p1(Lc, id_c, STENCIL_SHAPE_BOX); }
    interpolation_lists(Lf, id_f, 0.0, Lc, id_c, 17, 0x7);
  } else if (c.op == HPGMG_OP_27PT) {                           /* operators.27pt.c:150-151 -> interpolation_p2.c:228-230 */
    if (!hp_exchange_and_bcs_one_launch(Lc, id_c, STENCIL_SHAPE_BOX, 12, 1)) { exchange_boundary(Lc, id_c, STENCIL_SHAPE_BOX); apply_BCs_p2(Lc, id_c, STENCIL_SHAPE_BOX); }
    interpolation_lists(Lf, id_f, 0.0, Lc, id_c, 18, 0x7);
  } else if (c.op == HPGMG_OP_FV2) {                            /* operators.fv2.c:151-152 -> interpolation_v2.c:210-212 */
    if (!hp_exchange_and_bcs_one_launch(Lc, id_c, STENCIL_SHAPE_BOX, 2, 1)) { exchange_boundary(Lc, id_c, STENCIL_SHAPE_BOX); apply_BCs_v2(Lc, id_c, STENCIL_SHAPE_BOX); }
    interpolation_lists(Lf, id_f, 0.0, Lc, id_c, 19, 0x7);
  } else {                                                      /* interpolation_v4.c:276-278 */
    if (!hp_exchange_and_bcs_one_launch(Lc, id_c, STENCIL_SHAPE_BOX, 4, 1)) { exchange_boundary(Lc, id_c, STENCIL_SHAPE_BOX); apply_BCs_v4(Lc, id_c, STENCIL_SHAPE_BOX); }
    interpolation_lists(Lf, id_f, 0.0, Lc, id_c, 20, 0x7);
  }
  return 1;
}
void interpolation_fcycle(level_type *Lf, int id_f, double prescale, level_type *Lc, int id_c) {
  hpgmg_config c; hpgmg_get_config(&c);
  if (c.op == HPGMG_OP_27PT || c.op == HPGMG_OP_FV2) { hp_do_interpolation_vcycle(Lf, id_f, prescale, Lc, id_c); return; } /* operators.27pt.c:150-151, .fv2.c:151-152 */
  if (c.op == HPGMG_OP_FV4) {                                   /* interpolation_v4.c:276-278 */
    if (!hp_exchange_and_bcs_one_launch(Lc, id_c, STENCIL_SHAPE_BOX, 4, 1)) { exchange_boundary(Lc, id_c, STENCIL_SHAPE_BOX); apply_BCs_v4(Lc, id_c, STENCIL_SHAPE_BOX); }
    interpolation_lists(Lf, id_f, prescale, Lc, id_c, 4, 0x7);
    return;
  }
  if (c.op != HPGMG_OP_7PT) hp_no_kernel("interpolation_fcycle for this operator");
  /* interpolation_p1.c:71-72: the coarse operand's ghost zones are filled first -- exchange_boundary + apply_BCs_p1 as ONE launch where the level qualifies
   * (hp_exchange_and_bcs_one_launch: ghost-free mode, no messages, Dirichlet, every condition's sources local), otherwise the two operators (HPGMG_GHOST_FREE=0
   * always).  The interpolation kernel then reads every coarse neighbour from the ghost zone, as the reference does */
  if (!hp_exchange_and_bcs_one_launch(Lc, id_c, STENCIL_SHAPE_BOX, 1, 1)) { exchange_boundary(Lc, id_c, STENCIL_SHAPE_BOX); apply_BCs_p1(Lc, id_c, STENCIL_SHAPE_BOX); }
  interpolation_lists(Lf, id_f, prescale, Lc, id_c, 1, 0x7);
}

/* ---------------------------------------------------------------- misc.c */
void hp_do_zero_vector(level_type *L, int id) { hp_coef_written(L, id); BLAS1(hpgmg_hip_fill(&hp_backend_of(L)->dev, id, 0.0)); }
void init_vector(level_type *L, int id, double s) { hp_coef_written(L, id); BLAS1(hpgmg_hip_fill(&hp_backend_of(L)->dev, id, s)); }
void hp_do_add_vectors(level_type *L, int c, double sa, int a, double sb, int b) { hp_coef_written(L, c); BLAS1(hpgmg_hip_axpby(&hp_backend_of(L)->dev, c, sa, a, sb, b)); }
void hp_do_mul_vectors(level_type *L, int c, double s, int a, int b) { hp_coef_written(L, c); BLAS1(hpgmg_hip_mul(&hp_backend_of(L)->dev, c, s, a, b)); }
void invert_vector(level_type *L, int c, double s, int a) { hp_coef_written(L, c); BLAS1(hpgmg_hip_invert(&hp_backend_of(L)->dev, c, s, a)); }
void hp_do_scale_vector(level_type *L, int c, double s, int a) { hp_coef_written(L, c); BLAS1(hpgmg_hip_scale(&hp_backend_of(L)->dev, c, s, a)); }
void shift_vector(level_type *L, int c, int a, double shift) { hp_coef_written(L, c); BLAS1(hpgmg_hip_shift(&hp_backend_of(L)->dev, c, a, shift)); }
void color_vector(level_type *L, int id, int colors, int ic, int jc, int kc) { hp_coef_written(L, id); BLAS1(hpgmg_hip_color(&hp_backend_of(L)->dev, id, colors, ic, jc, kc)); }
void random_vector(level_type *L, int id) { hp_coef_written(L, id); BLAS1(hpgmg_hip_random(&hp_backend_of(L)->dev, id)); }

/* A launch of bricks (kernels/brick_visit.hip, brick_wide.hip) whose workgroups could not all run gives up after 2 s and raises an error word; every scalar the
 * host waits for passes hp_allreduce_scalar, which is where it learns of it.  Inside a solve the driver can repeat (hpgmg_solve_attempt_begin / _end, one
 * rank) the failure is noted, brick launches are switched off for the rest of the process and the driver repeats the solve launch by launch; anywhere else
 * -- the reference's own driver, several ranks (only rank 0 would know) -- the program stops with a message. */
static int attempt_open = 0, attempt_failed = 0;
static long long brick_failures = 0;
long long hpgmg_brick_failures(void) { return brick_failures; }      /* solves repeated launch by launch after a failed brick launch (tests) */
static const char *brick_failure_text = "hpgmg: an exchange inside a brick launch gave up after 2 s -- not all its workgroups were running (other processes' launches of this kind on "
                                        "the same GPU?).  Results since then are void.";
void hpgmg_solve_attempt_begin(void) {
  const hpgmg_transport *T = hpgmg_get_transport();
  attempt_open = !(T && T->size > 1);
  attempt_failed = 0;
}
static void brick_failure_noted(void) {
  attempt_failed = 1;
  brick_failures++;
  hp_switch_set(SW_BRICK_VISITS, 0);
  if (hpgmg_hip_brick_visit_error_clear()) { fprintf(stderr, "hpgmg: %s\n", hpgmg_hip_last_error()); abort(); }
}
int hpgmg_solve_attempt_end(void) {
  hp_lazy_flush();
  if (attempt_open && !attempt_failed && hpgmg_hip_brick_visit_error()) { if (hpgmg_hip_sync()) abort(); brick_failure_noted(); }
  attempt_open = 0;
  if (attempt_failed) {
    fprintf(stderr, "%s  Brick launches are off from here on (HPGMG_BRICK_VISITS=0); the solve is repeated launch by launch.\n", brick_failure_text);
    attempt_failed = 0;
    return 1;
  }
  return 0;
}
double hp_allreduce_scalar(level_type *L, double v, int op) { hp_allreduce_values(L, &v, 1, op); return v; }
void hp_allreduce_values(level_type *L, double *v, int n, int op) {
  const hpgmg_transport *T = hpgmg_get_transport();
  if (hpgmg_hip_brick_visit_error()) {
    if (!attempt_open) { fprintf(stderr, "%s  HPGMG_BRICK_VISITS=0 runs these levels launch by launch.\n", brick_failure_text); abort(); }
    if (!attempt_failed) brick_failure_noted();      /* (the value in hand is void; the driver throws the solve away at hpgmg_solve_attempt_end) */
  }
  if (T && T->size > 1) {
    hpgmg_level_ext *X = hpgmg_level_ext_get(L);
    if (X->num_active_ranks > 1) { const double t0 = hp_now(); T->allreduce(T->ctx, v, n, op, X->active_ranks, X->num_active_ranks); L->timers.collectives += hp_now() - t0; }   /* host-synchronous by nature: host clock in every mode */
  }
}
double hp_do_dot(level_type *L, int a, int b) { double v; BLAS1(hpgmg_hip_dot(&hp_backend_of(L)->dev, a, b, &v)); return hp_allreduce_scalar(L, v, HPGMG_REDUCE_SUM); }
double hp_do_norm(level_type *L, int a) {
  double v; BLAS1(hpgmg_hip_norm_max(&hp_backend_of(L)->dev, a, &v)); return hp_allreduce_scalar(L, v, HPGMG_REDUCE_MAX); }
double mean(level_type *L, int a) {
  double v; BLAS1(hpgmg_hip_sum(&hp_backend_of(L)->dev, a, &v));
  v = hp_allreduce_scalar(L, v, HPGMG_REDUCE_SUM);
  return v / (double)((double)L->dim.i * (double)L->dim.j * (double)L->dim.k);
}
double error(level_type *L, int a, int b) { add_vectors(L, VECTOR_TEMP, 1.0, a, -1.0, b); return norm(L, VECTOR_TEMP); }
