/*
 * hpgmg_mg.h -- multigrid hierarchy + cycle driver + bottom solver + transport.
 *
 * Callers of the operator plugin.  Same entry points as the reference's
 * mg.h:22-45 and solvers.h:8-9; the control flow of FMGSolve/MGVCycle follows
 * reference mg.c:1135-1344 call for call, because the order of operator calls
 * is what the golden residual norms pin.
 */
#ifndef HPGMG_MG_H
#define HPGMG_MG_H

#include "hpgmg_level.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MG_AGGLOMERATION_START 8     /* reference mg.h:15-16 */
#define MG_DEFAULT_BOTTOM_NORM 1e-3  /* reference mg.h:18-19 */

typedef struct {
  int my_rank;
  int num_levels;
  level_type **levels;
  struct { double MGBuild, MGSolve; } timers;
  int MGSolves_performed;
} mg_type;

void MGBuild(mg_type *all_grids, level_type *fine_grid, double a, double b, int minCoarseGridDim);
void MGDestroy(mg_type *all_grids);
/* MGBuild's last steps: rebuild_operator(level l, level l-1) for every coarser level, then must_subtract_mean of every level.  MGBuild runs it
 * once; a caller that gives the finest level new coefficients runs rebuild_operator(level 0, NULL) and then this. */
void MGRebuildCoarse(mg_type *all_grids, double a, double b);
/* MGRebuildCoarse for a caller whose walls need coefficients of the level's own (Robin walls: DESIGN.md §11.5).  Per level l >= 1, in order:
 * rebuild_operator(level l, level l-1), store_walls(ctx, all_grids, l), which writes level l's wall coefficients, rebuild_operator(level l, NULL);
 * level l+1 then restricts from the corrected level l.  Then must_subtract_mean of every level, as MGRebuildCoarse. */
void MGRebuildCoarseWalls(mg_type *all_grids, double a, double b, void (*store_walls)(void *ctx, mg_type *all_grids, int level), void *ctx);
void MGVCycle(mg_type *all_grids, int e_id, int R_id, double a, double b, int level);
void MGSolve(mg_type *all_grids, int onLevel, int u_id, int F_id, double a, double b, double rtol);
void FMGSolve(mg_type *all_grids, int onLevel, int u_id, int F_id, double a, double b, double rtol);
void hpgmg_set_ucycles(int on);        /* before MGBuild: 1 = the reference's -DUSE_UCYCLES ladder (boxes halved, never merged; mg.c:878-893) */
void hpgmg_fmg_zero_u_first(void);  /* the NEXT FMGSolve starts from u = 0: it zeroes u itself, where it first touches it (the benchmark step's zero_vector(u), hpgmg-fv.c:77-85) */
void hpgmg_set_fmg_vcycles(int n);     /* V-cycles FMGSolve may add after its F-cycle: 0 (default) or 20 = -DUNLIMIT_FMG_ITERATIONS (mg.c:1239-1247) */
/* F-cycle hook of the boundary-value solves (hpgmg_user_set_rhs_dirichlet); NULL (the default) leaves FMGSolve as it is.
 * While one is set, FMGSolve calls rhs_restricted(hook, G, l, R_id) after each restriction of the right-hand side onto level l >= 1, and its
 * own restriction chain and climb take the launch-by-launch forms (the V-cycles it runs keep every fused form).  key goes into the keys of
 * the captured segments, so a hooked and an unhooked F-cycle never share one. */
typedef struct hpgmg_fmg_hook {
  void (*rhs_restricted)(const struct hpgmg_fmg_hook *hook, mg_type *G, int level, int R_id);
  void (*interpolated)(const struct hpgmg_fmg_hook *hook, mg_type *G, int level, int e_id);
  void *ctx;
  long long key;
} hpgmg_fmg_hook;
void hpgmg_fmg_set_hook(const hpgmg_fmg_hook *hook);
void MGPCG(mg_type *all_grids, int onLevel, int x_id, int F_id, double a, double b, double rtol);   /* mg.c:1500-1605: CG preconditioned with one V-cycle per iteration; grows every level by three vectors */
/* CG on A u = F preconditioned with one V-cycle per iteration, for the user-problem API: Saad's algorithm 9.1 as MGPCG, but through the
 * fused passes hpgmg_pcg_* (include/hpgmg_operators.h) with their own summation order, up to max_iter iterations, and never aborting.  x_is_guess: start from
 * what x_id holds (else from 0).  Returns 1 when |F - A x|_inf < rtol |F|_inf, 0 after max_iter iterations or a breakdown (a zero or non-finite p.Ap, r.z,
 * alpha or beta): x is then the last iterate.  hpgmg_last_solve holds |F|, the TRUE residual norm of x and the number of V-cycles run (= iterations). */
int  MGPCGSolve(mg_type *all_grids, int onLevel, int x_id, int F_id, double a, double b, double rtol, int max_iter, int x_is_guess);
/* The flexible form (Notay's FCG truncated to one direction), for a preconditioner that is not one fixed linear operator -- a V-cycle whose
 * coarsest level BiCGStab solves to a tolerance (periodic boxes, N with an odd factor): MGPCGSolve except that after the V-cycle ONE pass, hpgmg_pcg_dot2,
 * returns r.z and Ap.z, and beta = -(Ap.z / p.Ap) makes the new direction A-orthogonal to the last one explicitly.  A beta of 0.0 is legitimate (p = z);
 * only a non-finite one ends the solve.  Arguments, vectors, return value and hpgmg_last_solve as MGPCGSolve. */
int  MGFPCGSolve(mg_type *all_grids, int onLevel, int x_id, int F_id, double a, double b, double rtol, int max_iter, int x_is_guess);
/* The V-cycle as a preconditioner for a driver outside host/mg.c (the eigen-solver of the user-problem API), exactly as the two CG solves
 * above call it: Begin once per solve (the launch-bound segments get a key of their own), then per application z = 0 and one V-cycle from onLevel on
 * A z = r, counted in vcycles_from_this_level.  z_id and r_id must be vectors of EVERY level (the cycle restricts and corrects under the same ids). */
void MGPreconditionerBegin(mg_type *all_grids, int onLevel, int z_id, int r_id, double a, double b);
void MGPreconditionerApply(mg_type *all_grids, int onLevel, int z_id, int r_id, double a, double b);
void MGPrintTiming(mg_type *all_grids, int fromLevel);
void MGResetTimers(mg_type *all_grids);
void richardson_error(mg_type *all_grids, int levelh, int u_id);

/* bottom solver (reference solvers.h / solvers/bicgstab.c) -- host control flow */
void IterativeSolver(level_type *level, int u_id, int f_id, double a, double b, double desired_reduction_in_norm);
int  IterativeSolver_NumVectors(void);

/* last values computed by FMGSolve/MGSolve/richardson_error -- what the
 * reference only prints (mg.c:1328, :1128, :1130); kept so tests can read them. */
typedef struct {
  double norm_of_F, norm_of_residual;   /* after the F-cycle (or last V-cycle) */
  double richardson_error, richardson_order;
  int    vcycles;
} hpgmg_solve_record;
extern hpgmg_solve_record hpgmg_last_solve;
extern int hpgmg_verbose;  /* 1 = print exactly what the reference prints (default), 0 = silent */

/* ---- transport: what replaces MPI (reference SURVEY 2.3) --------------------
 * One process per GPU.  Buffers handed to sendrecv live in plugin memory
 * (device pointers in the HIP build).  A NULL transport means one rank. */
enum { HPGMG_REDUCE_MAX = 0, HPGMG_REDUCE_SUM = 1 };
typedef struct {
  int   rank, size;
  void *ctx;
  /* post every receive and every send of one exchange phase and complete them
   * (MPI_Irecv* / MPI_Isend* / MPI_Waitall of reference exchange_boundary.c:33-97) */
  void (*sendrecv)(void *ctx,
                   int nrecv, double *const *rbuf, const int *rsize, const int *rrank,
                   int nsend, double *const *sbuf, const int *ssize, const int *srank, int tag);
  /* in-place allreduce of n host doubles over the listed ranks (sorted, includes caller) */
  void (*allreduce)(void *ctx, double *vals, int n, int op, const int *ranks, int nranks);
  /* optional (NULL: not wanted).  MGBuild calls it on EVERY rank of the job, in the same order, once per level whose reductions run over a proper
   * subset of the ranks (the reference's MPI_Comm_split per level, mg.c:985-993): a transport that can make a sub-communicator for the set does it
   * here -- building one is collective over the whole job (ncclCommSplit), which allreduce(), called by the members only, cannot be. */
  void (*prepare_subset)(void *ctx, const int *ranks, int nranks);
} hpgmg_transport;
void hpgmg_set_transport(const hpgmg_transport *t);
const hpgmg_transport *hpgmg_get_transport(void);

/* per-level side record (never stored inside level_type, see hpgmg_level.h) */
typedef struct hpgmg_level_ext {
  level_type *level;
  int  *active_ranks;      /* ranks that take part in reductions on this level */
  int   num_active_ranks;
  void *backend;           /* plugin-private (device mirrors of the block lists ...) */
  double *slab;            /* single allocation holding every owned box, or NULL */
  size_t  slab_doubles;
  struct hpgmg_level_ext *next;
} hpgmg_level_ext;
hpgmg_level_ext *hpgmg_level_ext_get(level_type *level);   /* creates on first use */
void             hpgmg_level_ext_drop(level_type *level);

#ifdef __cplusplus
}
#endif
#endif
