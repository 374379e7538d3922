/*
 * hpgmg_fv.h -- C-ABI of the host driver library (libhpgmg_fv.so / liboracle_fv.so).
 *
 * Plain pointers, ints and doubles only; this is what ctypes (tests, bench.py)
 * and any non-C host binds.  It wraps what the reference does in
 * finite-volume/source/hpgmg-fv.c: main() :103-386 (problem-size selection
 * :152-205, level creation :283-295, MGBuild :308, the timed loop :320-345,
 * Richardson analysis :351-366) and bench_hpgmg() :50-99.
 */
#ifndef HPGMG_FV_H
#define HPGMG_FV_H

#include "hpgmg_level.h"
#include "hpgmg_operators.h"
#include "hpgmg_mg.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct hpgmg_solver {
  level_type level_h;   /* finest level */
  mg_type    mg;
  double a, b, h;
  int boxes_in_i, box_dim;
  int my_rank, num_ranks;
} hpgmg_solver;

/* largest boxes_in_i with boxes_in_i^3 <= boxes_per_rank*ranks whose odd part of
 * (box_dim*boxes_in_i) is <= 11 (reference hpgmg-fv.c:181-197); -1 if none */
int hpgmg_choose_boxes_in_i(int log2_box_dim, int target_boxes_per_rank, int num_ranks);

/* create level + problem + operator + hierarchy (hpgmg-fv.c:283-308).
 * Call hpgmg_configure() first.  bc = BC_DIRICHLET or BC_PERIODIC. */
hpgmg_solver *hpgmg_solver_create(int log2_box_dim, int target_boxes_per_rank, int bc, int my_rank, int num_ranks);
/* same, but with an explicit box grid (tests use tiny domains the CLI rejects) */
hpgmg_solver *hpgmg_solver_create_explicit(int boxes_in_i, int box_dim, int bc, int my_rank, int num_ranks);
void hpgmg_solver_destroy(hpgmg_solver *s);

int         hpgmg_solver_num_levels(const hpgmg_solver *s);
level_type *hpgmg_solver_level(hpgmg_solver *s, int l);

/* F(l) = restriction of F(l-1), as the benchmark does before solving on 2h, 4h (hpgmg-fv.c:324) */
void   hpgmg_solver_restrict_rhs(hpgmg_solver *s, int l);
/* zero_vector(U); FMGSolve(...) on level l; returns ||F - A u||_inf (hpgmg-fv.c:79-81) */
double hpgmg_solver_fmg(hpgmg_solver *s, int l);
/* warmup + timed solves (hpgmg-fv.c:50-99); returns average seconds per solve */
double hpgmg_solver_bench(hpgmg_solver *s, int l, int warmup, int solves);
mg_type *hpgmg_solver_mg(hpgmg_solver *s);                               /* the hierarchy, for callers of MGSolve / FMGSolve (hpgmg_mg.h) */
void   hpgmg_solver_coefficients(const hpgmg_solver *s, double ab[2]);   /* the a, b of the test problem */
/* solve on l, l+1, l+2 then richardson_error (hpgmg-fv.c:351-366); out[0]=error out[1]=order */
void   hpgmg_solver_richardson(hpgmg_solver *s, double out[2]);

/* the reference's whole main(): prints the same report; returns 0 */
int hpgmg_fv_main(int argc, char **argv);

/* ---- user problems on dense arrays: the 7-point variable-coefficient operator  a alpha u - b div(beta grad u)  on an N^3 grid, one rank ----
 * Cell (i,j,k) has its centre at ((i+1/2)h, (j+1/2)h, (k+1/2)h).  Arrays are C-contiguous float64 indexed [k][j][i] (i fastest).  f, alpha, u,
 * u0, x, y: (N,N,N).  Dirichlet (homogeneous; the ghost rule of boundary_fd.c p1, as the plugin applies it): beta_i (N,N,N+1) with
 * beta_i[k][j][i] on the face between cells i-1 and i, so i = 0 and i = N are the domain faces; beta_j (N,N+1,N), beta_k (N+1,N,N).
 * Periodic: all three (N,N,N) (face N is face 0).  Poisson is a = 0 and has no alpha.  where: HPGMG_WHERE_HOST (host memory) or
 * HPGMG_WHERE_PLUGIN (the plugin's memory: a device array in the HIP build, read and written in place).  Every call returns HPGMG_USER_*.
 * The operator configuration is process-wide (hpgmg_configure): create refuses one that differs from a live user solver's. */
enum { HPGMG_USER_OK = 0, HPGMG_USER_BAD_ARGUMENT = -1, HPGMG_USER_CONFLICT = -2, HPGMG_USER_MULTI_RANK = -3, HPGMG_USER_NOT_FINITE = -4,
       HPGMG_USER_OUT_OF_RANGE = -5, HPGMG_USER_NOT_READY = -6, HPGMG_USER_UNSUPPORTED = -7 };
enum { HPGMG_USER_FMG = 0, HPGMG_USER_MG = 1, HPGMG_USER_PCG = 2, HPGMG_USER_FPCG = 3 };
typedef struct hpgmg_user_solver hpgmg_user_solver;
typedef struct {
  double norm_of_residual;   /* |f - A u|_inf (f after the mean shift) */
  double norm_of_f;          /* |f|_inf */
  double mean_shift;         /* what set_rhs subtracted from f (periodic without an a alpha term), else 0 */
  int    vcycles;            /* V-cycles run from the finest level (an F-cycle ends with one) */
  int    converged;          /* norm_of_residual < rtol * norm_of_f */
} hpgmg_user_info;
/* op must be HPGMG_OP_7PT (others: HPGMG_USER_UNSUPPORTED); box_dim <= 0: the largest power of two <= 128 dividing n; h <= 0: 1/n.
 * Configures {7pt, smoother, a != 0, variable coefficients}, sets every beta (and alpha) to 1 and f to 0, builds the hierarchy. */
int  hpgmg_user_create(int n, int box_dim, int bc, int op, int smoother, double a, double b, double h, hpgmg_user_solver **out);
void hpgmg_user_destroy(hpgmg_user_solver *s);
void hpgmg_user_set_verbose(hpgmg_user_solver *s, int on);      /* 1: print what the solver prints (default 0: nothing) */
hpgmg_solver *hpgmg_user_solver_of(hpgmg_user_solver *s);       /* its levels and hierarchy (hpgmg_solver_level, hpgmg_solver_mg) */
/* pack the coefficients (beta > 0, alpha >= 0, all finite), rebuild the operator on the finest level, then MGRebuildCoarse */
int  hpgmg_user_set_coefficients(hpgmg_user_solver *s, const double *alpha, const double *beta_i, const double *beta_j, const double *beta_k, int where);
/* pack f (finite); periodic without an a alpha term: subtract its mean, returned in *mean_shift */
int  hpgmg_user_set_rhs(hpgmg_user_solver *s, const double *f, int where, double *mean_shift);
/* HPGMG_USER_FMG: what the benchmark runs (zero u, FMGSolve); HPGMG_USER_MG: V-cycles until |f - A u| < rtol |f| (MGSolve).
 * u0 != NULL: u = u0 + e, where V-cycles solve A e = f - A u0 until |f - A u| < rtol |f| (method is then not read). */
int  hpgmg_user_solve(hpgmg_user_solver *s, int method, double rtol, const double *u0, int where, hpgmg_user_info *info);
/* HPGMG_USER_PCG: conjugate gradients on A u = f preconditioned with one V-cycle per iteration (MGPCGSolve), for coefficients with
 * jumps, on which V-cycles alone stall.  Starts from u0 when given (else 0) and runs until |f - A u| < rtol |f| or for set_max_iterations() iterations
 * (default 100; n < 1: HPGMG_USER_BAD_ARGUMENT; read by the two CG methods only).  It never aborts: after the last iteration or a breakdown info.converged is 0,
 * u the last iterate and info.norm_of_residual its true residual.  info.vcycles = preconditioner applications.  The hierarchy grows by three vectors
 * per level at the first such solve.  Boundary values need no F-cycle hook: it solves A0 u = f + T(g) as HPGMG_USER_MG does.
 * HPGMG_USER_FPCG: the same with the flexible beta = -(Ap.z / p.Ap) (MGFPCGSolve), which does not rely on the V-cycle being one fixed
 * symmetric operator.  It is not one where BiCGStab solves the coarsest level to its tolerance -- periodic boxes, N with an odd factor -- and there
 * HPGMG_USER_PCG can need many times the iterations or none that suffice; elsewhere the two take the same number.  One more fused inner product per
 * iteration, the same three vectors, the same u0, limits (set_max_iterations is read by both) and reporting. */
int  hpgmg_user_set_max_iterations(hpgmg_user_solver *s, int n);
int  hpgmg_user_get_solution(hpgmg_user_solver *s, double *u, int where);
int  hpgmg_user_apply(hpgmg_user_solver *s, const double *x, double *y, int where);   /* y = A x (apply_op) */
/* Inhomogeneous Dirichlet values.  g: (6,N,N) float64 of face-centre values, in the same memory as f / x (where): g[0], g[1]
 * the i-low / i-high faces indexed [k][j], g[2], g[3] j-low / j-high [k][i], g[4], g[5] k-low / k-high [j][i].  A boundary cell's ghost is
 * 2 g - u; the equations are A0 u = f + T(g), A0 the operator above (homogeneous ghosts), T of include/hpgmg_operators.h.
 * set_rhs_dirichlet: packs F = f + T(g) (f and g finite: else HPGMG_USER_NOT_FINITE) and the per-level g_l; the next HPGMG_USER_FMG solve runs an
 * F-cycle whose coarse right-hand sides carry each level's own T_l(g_l); HPGMG_USER_MG and u0 solve A0 u = F as they are.  set_rhs clears the
 * boundary values; set_coefficients after set_rhs_dirichlet leaves no right-hand side (solve: HPGMG_USER_NOT_READY).  info.norm_of_f is |F|.
 * apply_dirichlet: y = A0 x - T(g), the residual operator of the boundary-value problem.  A periodic solver: HPGMG_USER_UNSUPPORTED. */
int  hpgmg_user_set_rhs_dirichlet(hpgmg_user_solver *s, const double *f, const double *g, int where, double *mean_shift);
int  hpgmg_user_apply_dirichlet(hpgmg_user_solver *s, const double *x, const double *g, double *y, int where);
/* Neumann and mixed walls: hpgmg_user_create with one kind per domain face, in the order of g's faces (i-low, i-high, j-low,
 * j-high, k-low, k-high).  Six HPGMG_FACE_DIRICHLET is hpgmg_user_create(BC_DIRICHLET)'s solver.  On a Neumann face the ghost is u + h gn, gn the
 * OUTWARD normal derivative: the entry of g that set_rhs_dirichlet / apply_dirichlet take for that face (Dirichlet faces keep u's value).  The
 * beta arrays keep their Dirichlet shapes; a Neumann wall's beta (still > 0) weighs its data, phi = ((b * (1.0 / h)) * beta) * gn, and the operator
 * A_N has 0 there.  set_rhs on such a solver is set_rhs_dirichlet with zero data.  Six Neumann faces without an a alpha term: the constants are in
 * the null space, so set_rhs* subtracts the mean of f + T(g) (*mean_shift) and the solution is the mean-free one. */
/* bit 0: the wall is masked (its beta lives in the solver's wall array, not in the level's vector); bit 1: it carries a kappa.  2 alone is no kind. */
enum { HPGMG_FACE_DIRICHLET = 0, HPGMG_FACE_NEUMANN = 1, HPGMG_FACE_ROBIN = 3 };
int  hpgmg_user_create_faces(int n, int box_dim, const int face_bc[6], int op, int smoother, double a, double b, double h, hpgmg_user_solver **out);
/* Robin (convective) walls: HPGMG_FACE_ROBIN in face_bc makes that face a wall  du/dn + kappa u = g  (dn outward): the entry of g that
 * set_rhs_dirichlet / apply_dirichlet take for it is that g, and its ghost is ((2 - t) u + 2 h g) / (2 + t), t = kappa h.  kappa >= 0 comes with the
 * coefficients: set_coefficients_robin takes it as (6,N,N) doubles in g's layout and memory (where), copies it (the entries of faces that are not
 * Robin are not read: stored as 0) and keeps a restricted copy per level, since the wall's part of the diagonal depends on the level's h.  kappa not
 * finite: HPGMG_USER_NOT_FINITE, negative on a Robin face: HPGMG_USER_OUT_OF_RANGE.  A solver with a Robin face refuses the plain set_coefficients
 * (HPGMG_USER_BAD_ARGUMENT); one without takes set_coefficients_robin with kappa == NULL only, as set_coefficients.  kappa = 0 everywhere is the
 * Neumann wall bit for bit.  Six Neumann or Robin faces without an a alpha term are singular only if kappa is 0 everywhere; else nothing is subtracted. */
int  hpgmg_user_set_coefficients_robin(hpgmg_user_solver *s, const double *alpha, const double *beta_i, const double *beta_j, const double *beta_k,
                                       const double *kappa, int where);
/* Face fluxes of u: q = -b beta grad u on every face -- the heat flux, Darcy velocity or current density -- into three arrays of
 * the shapes of beta_i / beta_j / beta_k, positive towards increasing index: flux_i[k][j][i] on the face between cells i-1 and i, entries 0 and N of a
 * Dirichlet-shaped solver being the domain walls (periodic: face 0 lies between cell N-1 and cell 0).  With wq = b * (1.0 / h) an inner face holds
 * (wq * beta) * (u_lo - u_hi); a wall face what the wall's ghost gives (2 g - u on a Dirichlet wall, u + h g on a Neumann one, the Robin ghost), with
 * the wall's own beta and kappa on a Neumann / Robin wall, so that cell by cell  a alpha u + (1/h) sum_d (q_d[high face] - q_d[low face])  is what
 * apply_dirichlet(u, g) returns.  u, g and the outputs are in the same memory (where); g == NULL: zero data (a periodic solver takes no other:
 * HPGMG_USER_UNSUPPORTED).  u or a g entry not finite: HPGMG_USER_NOT_FINITE; after a refused set_coefficients: HPGMG_USER_NOT_READY.  Only the
 * solver's operand vector (apply's) is written: the solution, the right-hand side and the state of the last set_rhs stay as they were. */
int  hpgmg_user_flux(hpgmg_user_solver *s, const double *u, const double *g, double *flux_i, double *flux_j, double *flux_k, int where);
/* Coefficient sensitivities.  Write apply(u; g) for apply_dirichlet(u, g) = A0 u - T(g): it is affine in alpha, in every beta entry and
 * in a Neumann / Robin wall's own beta.  For a state u and an adjoint lam, G_p = d/dp sum_c lam_c apply(u; g)_c for every coefficient entry p, into
 * d_alpha (N,N,N) and d_beta_i / j / k in the shapes of the beta arrays.  With t = kappa h:
 *   alpha[c]: a u_c lam_c;   the face between cells lo and hi = lo + 1 (box-to-box and the periodic wrap included): (b/h^2) (u_lo - u_hi) (lam_lo - lam_hi);
 *   a Dirichlet wall face of cell c: (b/h^2) 2 (u_c - g) lam_c;   a Neumann / Robin wall face: (b/h) (2/(2 + t)) (kappa u_c - g) lam_c   (kappa = 0: Neumann).
 * None reads a beta.  If J depends on the solution u of A u = f + T(g) and A lam = dJ/du with homogeneous data, then dJ/dp = -G_p and dJ/df = lam
 * (also for the singular solvers, whose solve subtracts the mean of any right-hand side).  u, lam, g and the outputs are in the same memory (where);
 * g == NULL: zero data (a periodic solver takes no other: HPGMG_USER_UNSUPPORTED).  d_alpha must be given exactly when a != 0, the others always
 * (else HPGMG_USER_BAD_ARGUMENT).  u, lam or a g entry not finite: HPGMG_USER_NOT_FINITE; before the first set_coefficients (there
 * are no coefficient arrays yet) and after a refused one: HPGMG_USER_NOT_READY.  Only the solver's operand vector and the scratch vector apply writes are written: the solution, the right-hand side, the state of the last set_rhs
 * and a live march stay as they were. */
int  hpgmg_user_sensitivity(hpgmg_user_solver *s, const double *u, const double *lam, const double *g, double *d_alpha, double *d_beta_i, double *d_beta_j,
                            double *d_beta_k, int where);
/* Cell-centred conductivities: the coefficient as ONE (N,N,N) array kcell -- a conductivity, permeability or density per cell.  The
 * beta of a face between two cells (box-to-box and the periodic wrap included) is their mean -- mean = HPGMG_MEAN_HARMONIC (0): 2 lo hi / (lo + hi),
 * HPGMG_MEAN_ARITHMETIC (1): (lo + hi) / 2 -- and a domain wall face of any kind has its cell's own value.
 * set_cell_coefficients is set_coefficients_robin with those three face arrays, bit for bit, and every rule of it (alpha, kappa, the statuses, what it
 * ends and invalidates); kcell must be finite and > 0, and a mean that overflows is HPGMG_USER_NOT_FINITE, one that underflows to zero
 * HPGMG_USER_OUT_OF_RANGE; an unknown mean is HPGMG_USER_BAD_ARGUMENT.
 * cell_sensitivity is hpgmg_user_sensitivity with the chain rule through the mean: d_alpha as there, and d_k[c] = sum over the six faces of cell c of
 * G_face dbeta_face/dk_c (1 on a wall), evaluated at the kcell handed in (G reads no coefficient), so that dJ/dk = -d_k.  kcell is validated as
 * set_cell_coefficients validates it.  Statuses and what is left untouched: hpgmg_user_sensitivity's. */
int  hpgmg_user_set_cell_coefficients(hpgmg_user_solver *s, const double *alpha, const double *kcell, int mean, const double *kappa, int where);
int  hpgmg_user_cell_sensitivity(hpgmg_user_solver *s, const double *u, const double *lam, const double *kcell, int mean, const double *g, double *d_alpha,
                                 double *d_k, int where);
/* Implicit time stepping:  alpha du/dt = b div(beta grad u) + f  with the walls and data g of the solver, by the theta scheme
 *   alpha (u1 - u0) / dt = theta w1 + (1 - theta) w0,   w = f - L(u; g) = alpha du/dt,   L(u; g) = apply_dirichlet(u, g) - a alpha u,
 * 1/2 <= theta <= 1 (1: backward Euler, 1/2: Crank-Nicolson).  One step is one solve with the operator for a = 1 / (theta dt).  The library keeps the
 * state u and the rate w on the device between calls; only f (and g) come in per step.
 * set_shift: a new a (> 0, finite) for a solver created with a != 0 (else HPGMG_USER_BAD_ARGUMENT): every level's operator is rebuilt from the
 *   coefficients set_coefficients left, without packing one; then as a solver created with that a and given the same coefficients, bit for bit.
 *   A right-hand side set before stays valid.
 * start: begins a march at u with the source f and data g of that time (g NULL as set_rhs allows it), sets a = 1 / (theta dt) and w = f - L(u; g).
 *   dt <= 0, theta outside [1/2, 1], a Poisson solver: HPGMG_USER_BAD_ARGUMENT; alpha zero everywhere: HPGMG_USER_UNSUPPORTED.  The first start gives
 *   the finest level two more vectors.  A start ends the march before it, also when it is refused (the state vector is packed first): after a
 *   refused start there is no march until one succeeds.
 * step: one step to the next time, f and g being those of the NEW time; dt, theta <= 0: as in the call before (a change sets the shift; w stays
 *   valid).  V-cycles from the state run until |F - A u| < rtol |F| (20 at most), F the right-hand side f + T(g) + a alpha u0 + c w0, c = (1 - theta) / theta;
 *   info as hpgmg_user_solve fills it (norm_of_f = |F|), *rate = max |w|.  w is exact for the u the solve stopped at, whatever rtol.  f or g not finite:
 *   HPGMG_USER_NOT_FINITE, and u, w and the march are as before the call.  Without a live march: HPGMG_USER_NOT_READY.
 * get_rate: w into an (N,N,N) array.  get_solution returns the state u.
 * set_coefficients*, set_rhs* and solve end a march (step: HPGMG_USER_NOT_READY until the next start); get_solution, apply*, flux, sensitivity and set_shift do
 * not.  After a step the solver holds no right-hand side of the caller's: solve needs a set_rhs first. */
int  hpgmg_user_set_shift(hpgmg_user_solver *s, double a);
int  hpgmg_user_start(hpgmg_user_solver *s, const double *u, const double *f, const double *g, int where, double dt, double theta);
int  hpgmg_user_step(hpgmg_user_solver *s, const double *f, const double *g, int where, double dt, double theta, double rtol, hpgmg_user_info *info,
                     double *rate);
int  hpgmg_user_get_rate(hpgmg_user_solver *s, double *out, int where);
/* Eigenmodes: the k smallest lambda of  K x = lambda M x,  K = -b div(beta grad .) with the solver's walls and homogeneous data (the
 * operator of hpgmg_user_apply without its a alpha term), M = diag(alpha) on a Helmholtz solver (a != 0) and M = I on a Poisson solver, by LOBPCG with
 * block size m = k + extra (1 <= k, 0 <= extra, m <= HPGMG_USER_EIGS_MAX_BLOCK, else HPGMG_USER_BAD_ARGUMENT) preconditioned with one V-cycle per active
 * column and iteration.  A Helmholtz solver iterates on A = a M + K with the shift a in force (set_shift's or a march's): its pencil eigenvalues are
 * mu = a + lambda > 0, lam[j] = mu_j - a (lambda loses digits when a >> lambda: set_shift moves a) and info->mu[j] = mu_j.
 * x0: m start vectors, an (m,N,N,N) array in `where` (not finite: HPGMG_USER_NOT_FINITE), or NULL: a deterministic start (products of low-order
 * polynomials in x, y, z plus a hash of the global cell index): the same call twice gives the same bits.  lam: k doubles on the HOST, ascending.
 * modes: (k,N,N,N) in `where`, mode j normalised to h^3 x^T M x = 1; its sign, and the basis within a degenerate cluster, are unspecified.
 * info: iterations, the V-cycles run, residuals[j] = max |A x_j - mu_j M x_j| / (mu_j max |M x_j|) of the returned pairs (true ones: from A x_j applied at
 * the end), mu, and converged = every residual < rtol.  Stopping short (max_iter, or a Rayleigh-Ritz step that broke down) is not an error: the last block
 * is returned with converged = 0.
 * Refused: a singular solver (periodic, or six Neumann / zero-kappa Robin walls, with a = 0 or alpha = 0: HPGMG_USER_UNSUPPORTED -- create the solver with
 * a > 0 and alpha = 1, the constant mode then comes back as lambda ~ 0); a Helmholtz solver with alpha == 0 in some cell (HPGMG_USER_OUT_OF_RANGE: M must
 * be positive definite); no valid coefficients (HPGMG_USER_NOT_READY).  A refusal writes nothing to lam, modes or info.
 * The coefficients stay as they are.  The call ends a live march and invalidates the stored right-hand side and solution, as set_coefficients does: solve
 * needs a set_rhs first.  The first call gives every level the three vectors of HPGMG_USER_PCG and the finest level 6 m more (a later call with a larger
 * m the difference). */
#define HPGMG_USER_EIGS_MAX_BLOCK 12
typedef struct {
  int iterations, vcycles, converged, reserved_;
  double residuals[HPGMG_USER_EIGS_MAX_BLOCK], mu[HPGMG_USER_EIGS_MAX_BLOCK];
} hpgmg_user_eig_info;
int  hpgmg_user_eigs(hpgmg_user_solver *s, int k, int extra, double rtol, int max_iter, const double *x0, int where, double *lam, double *modes,
                     hpgmg_user_eig_info *info);
/* The wave equation:  alpha d2u/dt2 + sigma alpha du/dt = b div(beta grad u) + f  with the walls and data g of the solver, by the
 * implicit Newmark rule (beta, gamma), gamma >= 1/2 and beta >= gamma / 2: the unconditionally stable rules (1/4, 1/2 is the average-acceleration
 * rule: second order, energy conserving).  One step is one solve with the operator for a = 1 / (beta dt^2) + sigma gamma / (beta dt), warm-started from
 * the predictor.  The library keeps u, v = du/dt and the acceleration q = d2u/dt2 on the device between calls; only f (and g) come in per step.
 * wave_start: begins a march at (u, v) with the source f and data g of that time (g NULL as set_rhs allows it), sets a and
 *   q = (f - L(u; g)) / alpha - sigma v.  dt <= 0 or not finite, sigma < 0 or not finite, gamma < 1/2, beta < gamma / 2, a not finite, a Poisson solver:
 *   HPGMG_USER_BAD_ARGUMENT; alpha == 0 in some cell: HPGMG_USER_OUT_OF_RANGE; g on a periodic box: HPGMG_USER_UNSUPPORTED; u, v, f or g not finite:
 *   HPGMG_USER_NOT_FINITE.  It shares hpgmg_user_start's two vectors and adds one more to the finest level at the first call.  It ends whatever march was
 *   live, also when it is refused after its first pack.  info: t = 0, vcycles = 0, norm_of_f = |f + T(g)|, norm_of_residual = |f + T(g) - A0 u|.
 * wave_step: one step to the next time, f and g being those of the NEW time; dt <= 0: as in the call before (a change sets the shift and nothing else;
 *   beta, gamma and sigma are wave_start's).  V-cycles from the predictor run until |F - A0 u| < rtol |F| (20 at most), F the step's right-hand side.
 *   f or g not finite: HPGMG_USER_NOT_FINITE, and u, v, q and the march are as before the call.
 * info: hpgmg_user_info's fields of the step's solve, t the time since wave_start, kinetic = h^3/2 sum alpha v^2 and potential = h^3/2 u^T K u
 *   (K = apply without its a alpha term and with zero data), the latter from the solve's closing residual: exact for the u the solve stopped at.
 * get_velocity, get_acceleration: v, q into an (N,N,N) array; get_solution returns u.
 * Only one march is live: hpgmg_user_step / _get_rate answer HPGMG_USER_NOT_READY on a wave march, the wave calls on a theta march or none.  Whatever
 * ends a theta march ends a wave march; after a step the solver holds no right-hand side of the caller's. */
typedef struct {
  double norm_of_residual, norm_of_f, mean_shift;
  int    vcycles, converged;
  double t, kinetic, potential;
} hpgmg_user_wave_info;
int  hpgmg_user_wave_start(hpgmg_user_solver *s, const double *u, const double *v, const double *f, const double *g, int where, double dt, double beta,
                           double gamma, double damping, hpgmg_user_wave_info *info);
int  hpgmg_user_wave_step(hpgmg_user_solver *s, const double *f, const double *g, int where, double dt, double rtol, hpgmg_user_wave_info *info);
int  hpgmg_user_get_velocity(hpgmg_user_solver *s, double *out, int where);
int  hpgmg_user_get_acceleration(hpgmg_user_solver *s, double *out, int where);

/* ---- small accessors so a ctypes caller never needs the struct layouts ---- */
enum { HPGMG_INFO_DIM = 0, HPGMG_INFO_BOX_DIM, HPGMG_INFO_GHOSTS, HPGMG_INFO_JSTRIDE, HPGMG_INFO_KSTRIDE,
       HPGMG_INFO_VOLUME, HPGMG_INFO_NUM_MY_BOXES, HPGMG_INFO_NUM_VECTORS, HPGMG_INFO_BOXES_IN_I,
       HPGMG_INFO_MY_RANK, HPGMG_INFO_NUM_RANKS, HPGMG_INFO_NUM_MY_BLOCKS, HPGMG_INFO_ACTIVE, HPGMG_INFO_COUNT };
void   hpgmg_level_info(const level_type *level, int out[HPGMG_INFO_COUNT]);
double hpgmg_level_h(const level_type *level);
double hpgmg_level_eigenvalue(const level_type *level);
int    hpgmg_level_must_subtract_mean(const level_type *level);      /* 1: the cycles keep this level's vectors mean-free (a singular operator); -1: not decided yet */
void   hpgmg_level_set_eigenvalue(level_type *level, double dominant_eigenvalue_of_DinvA);   /* what rebuild_operator would have left (tests of a Chebyshev smoother on given coefficients) */
void   hpgmg_level_box_low(const level_type *level, int box, int out[3]);
int    hpgmg_level_list_counts(const level_type *level, int which, int shape_or_type, int out[3]);
/* entry n of phase 0 / 1 / 2 of the same list (which 3: the boundary list, phase ignored): out = dim.i, dim.j, dim.k, read.box, read.i, read.j, read.k,
 * write.box, write.i, write.j, write.k.  Returns 0, or -1 where there is no such entry (out untouched) */
int    hpgmg_level_list_entry(const level_type *level, int which, int shape_or_type, int phase, int n, int out[11]);
/* whole padded box volume of one vector <-> host array of box_volume doubles */
void   hpgmg_level_read_vector(level_type *level, int box, int id, double *host_out);
void   hpgmg_level_write_vector(level_type *level, int box, int id, const double *host_in);
/* standalone level for operator-level tests */
level_type *hpgmg_level_create(int boxes_in_i, int box_dim, int ghosts, int numVectors, int bc, int my_rank, int num_ranks, double h);
void        hpgmg_level_destroy(level_type *level);
/* two-level hierarchy around an existing fine level (restriction/interpolation tests) */
mg_type    *hpgmg_mg_create(level_type *fine, double a, double b, int minCoarseDim);
void        hpgmg_mg_destroy(mg_type *mg);
level_type *hpgmg_mg_level(mg_type *mg, int l);
int         hpgmg_mg_num_levels(const mg_type *mg);
void        hpgmg_set_verbose(int v);
/* HIP build only: install the RCCL transport (id from hpgmg_hip_rccl_unique_id on rank 0) */
int         hpgmg_transport_init_rccl(const char *id128, int rank, int size);
void        hpgmg_transport_finalize_rccl(void);
/* the node-local peer-copy transport (hipIpc memory handles + stream-ordered host functions on shared counters, include/hpgmg_hip.h): `name` = a POSIX shared-memory
 * name ("/...") every rank of the job passes; rank 0 creates the segment */
int         hpgmg_transport_init_ipc(const char *name, int rank, int size);
void        hpgmg_transport_finalize_ipc(void);
/* first contact of a multi-rank job (every rank calls it once the transport is installed, before creating levels): a known pattern to and from every
 * other rank, one maximum, one rank-ordered sum, one sum over a rank subset, all checked; 0, -1 with the failing rank pair / reduction in msg, or -2 when only another rank saw a failure */
int         hpgmg_transport_selftest(char *msg, int msglen);
void        hpgmg_set_sync_timers(int on);
void        hpgmg_print_switches(void);        /* every run-time switch of the plugin (environment variable, value in force, default, meaning) on stderr; HPGMG_SWITCHES=1 prints it at load time */
void        hpgmg_set_small_fused(int mode);   /* 27-pt / fv2 / fv4: 2 (default) smooth() on levels of ONE box as one single-workgroup launch on an image of the box in LDS; 0 off */
void        hpgmg_set_small_vtail(int on);     /* 27-pt / fv2 / fv4: the rest of a V-cycle below a level of one box as ONE launch: 2 (default) on except for 27-pt GSRB, 1 on, 0 off; bit-identical */
void        hpgmg_set_small_ops(int on);       /* 1 (default): BLAS-1 calls / apply_op / residual on a level of one small box wait for the dot product or norm that
                                                  follows and go out with it as one launch (host-driven Krylov solvers); 0: a launch each */
long long   hpgmg_small_ops_groups(void);      /* such launches so far (tests) */
long long   hpgmg_small_ops_prefetched(void);  /* scalars answered from a value the previous launch formed in advance (tests) */
void        hpgmg_set_fused_bottom(int on);    /* 0: the bottom solve driven from the host (BiCGStab of host/solvers.c through the operators; tests) */
void        hpgmg_set_fused_tail(int on);      /* 0: no single-launch V-/F-cycle tails (7-pt: kernels/tail.hip; tests) */
void        hpgmg_set_brick_visits(int on);    /* 0: the 32^3 / 64^3 levels of a 7-pt V-cycle launch by launch instead of one launch per visit (kernels/brick_visit.hip); 1: on; 8 / 16: on, bricks of that side (tests) */
long long   hpgmg_brick_visits(void);          /* level visits done that way so far (tests) */
long long   hpgmg_brick_failures(void);        /* solves repeated launch by launch because a brick launch did not get all its workgroups running (tests) */
long long   hpgmg_brick_capacity_refusals(void);      /* level visits left to the launch-by-launch path because the device does not hold that many bricks at once (tests) */
void        hpgmg_set_brick_wide(int on);      /* 0: the 27-point / fv4 plugins visit their launch-bound levels launch by launch (kernels/brick_wide.hip off; tests) */
void        hpgmg_set_brick_chains(int on);    /* 0: one launch per level visit instead of one per V-cycle leg (tests) */
long long   hpgmg_pair_remote_smooths(void);   /* smooth() calls executed as sweep pairs with faces owned by other ranks (tests) */
long long   hpgmg_fp32_pair_smooths(void);     /* smooth() calls run on fp32-rounded coefficients (smoother precision 32): HIP, as sweep pairs reading the fp32
                                                  copies; the CPU oracle, the same calls on rounded copies (tests) */
void        hpgmg_set_pair_form_dinv(int on);  /* 7-pt sweep pairs: 1 = form Dinv in registers from the coefficient streams where VECTOR_DINV is known to be rebuild_operator's output for the
                                                  same a, b (bit-identical; HPGMG_PAIR_FORM_DINV), 0 = always read the vector */
long long   hpgmg_pair_formed_dinv_launches(void);     /* sweep-pair launches that formed Dinv so far (tests; a postponed smooth() is issued first) */
void        hpgmg_set_uniform_alpha(int on);   /* 7-pt Helmholtz: 1 = where rebuild_operator found alpha to be one bit pattern over every interior cell of the level, the sweep pairs that
                                                  form Dinv and the wide fused residual passes take it from their arguments instead of reading VECTOR_ALPHA (bit-identical;
                                                  HPGMG_UNIFORM_ALPHA), 0 = always read the vector */
long long   hpgmg_uniform_alpha_launches(void);        /* sweep-pair and fused residual launches that took alpha from their arguments so far (tests; postponed operators are issued first) */
long long   hpgmg_fused_residuals_remote(void); /* 7-point: fused residual passes (residual + restriction, residual + norm) run on levels with faces owned by other ranks (tests) */
long long   hpgmg_fv4_rb_smooths(void);        /* fv4: smooth() calls run as one-pass red + black sweeps; hpgmg_rb27_passes(): such passes of the 27-point smoother (tests) */
long long   hpgmg_rb27_passes(void);
long long   hpgmg_image_exchanges(void);       /* 27-point / fv4 across ranks: refreshes of the images of the neighbouring ranks' boxes (tests) */
/* level->timers after settling pending device timers: smooth, residual, apply_op, blas1, boundary_conditions, restriction_total,
 * interpolation_total, ghostZone_total, Total (seconds since MGResetTimers; reference level.h:162-196) */
void        hpgmg_level_timers(level_type *level, double out[9]);
void        hpgmg_set_gather_dim(int dim);  /* multi-rank: levels of <= dim^3 cells live entirely on rank 0 (default 64; 0 = the reference's rank map); call before MGBuild */
long long   hpgmg_overlap_count(void);      /* number of overlapped exchanges performed so far */
void        hpgmg_set_overlap(int on);      /* multi-rank: 1 (default) overlaps the halo exchange with the stencil launch that consumes it */
void        hpgmg_set_smoother_precision(int bits); /* 64 (default, bit-exact) or 32: mixed-precision Chebyshev smoother, BASELINE config 5 */
int         hpgmg_get_smoother_precision(void);
void        hpgmg_set_graphs(int on);       /* 1: replay the launch-bound segments of a cycle as hipGraphs (default 0: eager launches measured faster) */
void        hpgmg_set_fused_sweeps(int on); /* 1 (default): Chebyshev smooth() on boxes of side 128k runs as fused sweep pairs; 0: one launch per sweep */
void        hpgmg_set_pair_min_cells(long long cells); /* the smallest level (cells) that takes the sweep-pair kernel (default 2 000 000, HPGMG_PAIR_MIN_CELLS); tests */
void        hpgmg_set_ghost_free(int on);   /* 1 (default): fused ghost handling in the 7-pt stencil launches; 0: exchange + BC + stencil */
void        hpgmg_set_box_alignment(int jstride, int kstride, int volume, int base_bytes);

#ifdef __cplusplus
}
#endif
#endif
