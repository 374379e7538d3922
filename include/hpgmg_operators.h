/*
 * hpgmg_operators.h -- the operator plugin surface (THE drop-in boundary).
 *
 * Every prototype below has the same name, argument order and meaning as the
 * reference's finite-volume/source/operators.h:14-50.  The reference selects
 * one plugin (operators.7pt.c, .27pt.c, .fv4.c ...) and one smoother at compile
 * time with -D flags; here the same choices are a process-wide runtime
 * configuration (hpgmg_configure) because the reference's own
 * stencil_get_radius()/stencil_get_shape() take no level argument.
 *
 * Two implementations of this header exist in the repository:
 *   hpgmg_amd/csrc/host/operators_hip.c  -- product: forwards to the HIP kernels
 *                                           behind include/hpgmg_hip.h
 *   oracle/operators_cpu.c               -- test oracle: plain C restatement
 * They are never linked into the same binary.
 */
#ifndef HPGMG_OPERATORS_H
#define HPGMG_OPERATORS_H

#include "hpgmg_level.h"

#ifdef __cplusplus
extern "C" {
#endif

/* vector ids (reference defines.h:12-39).  ALPHA/L1INV exist only when the
 * configuration is Helmholtz, exactly like -DUSE_HELMHOLTZ in the reference. */
#define VECTOR_TEMP    0
#define VECTOR_U       1
#define VECTOR_F       2
#define VECTOR_E       3
#define VECTOR_R       4
#define VECTOR_DINV    5
#define VECTOR_BETA_I  6
#define VECTOR_BETA_J  7
#define VECTOR_BETA_K  8
#define VECTOR_ALPHA   9
#define VECTOR_L1INV  10

/* ---- runtime replacement of the reference's compile-time -D switches ---- */
enum { HPGMG_OP_7PT = 0, HPGMG_OP_27PT = 1, HPGMG_OP_FV4 = 2, HPGMG_OP_FV2 = 3 };
enum { HPGMG_SMOOTH_CHEBY = 0, HPGMG_SMOOTH_GSRB = 1, HPGMG_SMOOTH_JACOBI = 2 };

typedef struct {
  int op;                 /* HPGMG_OP_*          (which operators.X.c)             */
  int smoother;           /* HPGMG_SMOOTH_*      (-DUSE_CHEBY / -DUSE_GSRB / ...)   */
  int helmholtz;          /* 1 = -DUSE_HELMHOLTZ (adds VECTOR_ALPHA, VECTOR_L1INV) */
  int variable_coeff;     /* 1 = STENCIL_VARIABLE_COEFFICIENT (7pt/fv2/fv4)        */
} hpgmg_config;

/* Returns 0, or -1 for a combination the reference itself rejects with #error
 * (e.g. 27pt + variable coefficients, operators.27pt.c:53-55). */
int  hpgmg_configure(const hpgmg_config *cfg);
void hpgmg_get_config(hpgmg_config *cfg);
int  hpgmg_vectors_reserved(void); /* VECTORS_RESERVED: 9, or 11 for Helmholtz */
/* the reference's -DUSE_BICGSTAB / -DUSE_CG / -DUSE_CABICGSTAB / -DUSE_CACG (solvers.c:17-24): host loops over the operators.  The two CA (s-step)
 * solvers are the reference's defaults for them: CA_KRYLOV_S 4, telescoping CABiCGStab, no diagonal preconditioning.  Any other value selects BiCGStab. */
enum { HPGMG_BOTTOM_BICGSTAB = 0, HPGMG_BOTTOM_CG = 1, HPGMG_BOTTOM_CABICGSTAB = 2, HPGMG_BOTTOM_CACG = 3 };
void hpgmg_set_bottom_solver(int which);   /* before MGBuild (the solver's work vectors are created there: 8 / 5 / 20 / 12) */
int  hpgmg_get_bottom_solver(void);

/* ---- operators.h:14-15 ---- */
int stencil_get_radius(void);
int stencil_get_shape(void);
/* ---- operators.h:17-21 ---- */
void apply_op(level_type *level, int Ax_id, int x_id, double a, double b);
void residual(level_type *level, int res_id, int x_id, int rhs_id, double a, double b);
void smooth(level_type *level, int phi_id, int rhs_id, double a, double b);
void rebuild_operator(level_type *level, level_type *fromLevel, double a, double b);
void rebuild_operator_blackbox(level_type *level, double a, double b, int colors_in_each_dim);
/* ---- operators.h:23-25 ---- */
void restriction(level_type *level_c, int id_c, level_type *level_f, int id_f, int restrictionType);
void interpolation_vcycle(level_type *level_f, int id_f, double prescale_f, level_type *level_c, int id_c);
void interpolation_fcycle(level_type *level_f, int id_f, double prescale_f, level_type *level_c, int id_c);
/* ---- operators.h:27-33 ---- */
void exchange_boundary(level_type *level, int id_a, int shape);
void apply_BCs(level_type *level, int x_id, int shape);   /* plugin's dispatch, operators.7pt.c:47 */
void apply_BCs_p1(level_type *level, int x_id, int shape);
void apply_BCs_p2(level_type *level, int x_id, int shape);
void apply_BCs_v1(level_type *level, int x_id, int shape);
void apply_BCs_v2(level_type *level, int x_id, int shape);
void apply_BCs_v4(level_type *level, int x_id, int shape);
void extrapolate_betas(level_type *level);
/* ---- operators.h:35-45 ---- */
double dot(level_type *level, int id_a, int id_b);
/* solvers/matmul.c:6-62: C[mm * cols + nn] = dot(id_A[mm], id_B[nn]) for nn >= mm, mirrored to C[nn * cols + mm] where that entry exists (the
 * CA solvers pass id_A == id_B; A_equals_B_transpose is accepted and, as in the reference, not read), then ONE allreduce of the whole rows x cols
 * matrix.  Order of each entry: per box one chain over its dim^3 interior cells in k, j, i order, products a * b formed first, starting from 0.0;
 * the box partials added in box order 0 .. num_my_boxes - 1, starting from 0.0 -- NOT dot()'s per-tile order.  host/solvers.c defines a weak
 * default (boxes downloaded through hpgmg_vector_download, summed on the host); the HIP plugin overrides it with one Gram launch. */
void matmul(level_type *level, double *C, int *id_A, int *id_B, int rows, int cols, int A_equals_B_transpose);
double norm(level_type *level, int id_a);
double mean(level_type *level, int id_a);
double error(level_type *level, int id_a, int id_b);
void add_vectors(level_type *level, int id_c, double scale_a, int id_a, double scale_b, int id_b);
void scale_vector(level_type *level, int id_c, double scale_a, int id_a);
void zero_vector(level_type *level, int id_a);
void shift_vector(level_type *level, int id_c, int id_a, double shift_a);
void mul_vectors(level_type *level, int id_c, double scale, int id_a, int id_b);
void invert_vector(level_type *level, int id_c, double scale_a, int id_a);
void init_vector(level_type *level, int id_a, double scalar);
/* ---- operators.h:47-48 ---- */
void color_vector(level_type *level, int id, int colors, int icolor, int jcolor, int kcolor);
void random_vector(level_type *level, int id);
/* ---- operators.h:50 ---- */
void initialize_problem(level_type *level, double hLevel, double a, double b);

/* ---- the one hook outside operators.h: who owns vector storage -----------
 * The reference allocates with MALLOC() in level.c:25-40 and zero-fills on the
 * host (level.c:976).  The plugin supplies these instead, so level.c never
 * touches vector bytes: HIP build -> hipMalloc/hipMemset, oracle -> calloc. */
double *hpgmg_vector_alloc(size_t num_doubles);           /* zero-filled */
void    hpgmg_vector_free(double *p);
void    hpgmg_vector_copy(double *dst, const double *src, size_t num_doubles);
/* host<->plugin staging, used by tests and by initialize_problem */
void    hpgmg_vector_upload(double *dst_plugin, const double *src_host, size_t num_doubles);
void    hpgmg_vector_download(double *dst_host, const double *src_plugin, size_t num_doubles);
/* Dense N^3 arrays <-> vector `id` of a level (one rank; the user-problem API of include/hpgmg_fv.h).  A dense array is C-contiguous
 * float64 indexed [k][j][i] (i fastest); cell (i,j,k) is the cell whose global index is (i,j,k).  Layout HPGMG_DENSE_CELL: (N,N,N).
 * HPGMG_DENSE_FACE_I/J/K: the LOW face of cell (i,j,k) along that axis (hpgmg_level.h); with Dirichlet boundaries the array is one longer along
 * that axis (beta_i is (N,N,N+1)), its entry N being the high domain face; with periodic ones it is (N,N,N) (face N is face 0).
 * pack: every padded cell of every box is written -- the array's value where the array determines it (interior cells; for a Dirichlet face
 * array also the high ghost layer along its axis of the boxes on the domain's high face), 0.0 elsewhere; exchange_boundary fills the ghost
 * zones afterwards.  Each value is checked while it is copied: the result is 0, or HPGMG_DENSE_NOT_FINITE | HPGMG_DENSE_OUT_OF_RANGE (check
 * POSITIVE: v > 0, NONNEGATIVE: v >= 0) -- the vector is then written but not to be used -- or -1 for an argument the plugin refuses.
 * unpack: the interior cells of the vector into a (N,N,N) array; nothing else of the array is written.  where: HPGMG_WHERE_HOST = the array
 * is in host memory, HPGMG_WHERE_PLUGIN = in the plugin's memory (device memory in the HIP build; read and written in place).
 * host/hooks_host.inc holds weak host defaults (box by box through hpgmg_vector_upload / download: the CPU oracle); the HIP plugin overrides them
 * with one launch per array (kernels/dense_io.hip). */
enum { HPGMG_DENSE_CELL = 0, HPGMG_DENSE_FACE_I = 1, HPGMG_DENSE_FACE_J = 2, HPGMG_DENSE_FACE_K = 3 };
enum { HPGMG_DENSE_CHECK_FINITE = 0, HPGMG_DENSE_CHECK_POSITIVE = 1, HPGMG_DENSE_CHECK_NONNEGATIVE = 2 };
enum { HPGMG_DENSE_NOT_FINITE = 1, HPGMG_DENSE_OUT_OF_RANGE = 2 };
enum { HPGMG_WHERE_HOST = 0, HPGMG_WHERE_PLUGIN = 1 };
int     hpgmg_dense_pack(level_type *level, int id, const double *src, int where, int layout, int check);
int     hpgmg_dense_unpack(level_type *level, int id, double *dst, int where);
/* Inhomogeneous Dirichlet values (the boundary-value solves of include/hpgmg_fv.h).  A level's boundary array is 6 x n x n
 * doubles in the plugin's memory, n the level's cells per side: [0], [1] the i-low / i-high domain faces indexed [k][j]; [2], [3] j-low / j-high
 * indexed [k][i]; [4], [5] k-low / k-high indexed [j][i] (entry [q][p]: p the faster index).  The ghost of a boundary cell is 2 g - u instead of
 * -u, which moves  phi = ((2.0 * b) * (1.0 / (h * h))) * beta_face) * g  per face to the right-hand side: beta_face is the level's beta of that
 * face (beta_i at i = 0 of a box on the i-low face, at its high ghost layer i = dim on the i-high face; j, k alike), h the level's.  For a cell c
 * T(c) = 0.0 + phi of each domain face c touches, added in the order i-low, i-high, j-low, j-high, k-low, k-high.  Cells on no face: T = 0.
 *   pack_lifted:       vector id := f + T(c) from g (hpgmg_dense_pack's CELL layout and one pass; f and g are checked: HPGMG_DENSE_NOT_FINITE)
 *   boundary_flux:     phi of every entry of g (the level's beta, h; b) into phi; returns HPGMG_DENSE_NOT_FINITE if g holds a non-finite value
 *   boundary_restrict: g_c[f][q][p] = (g_f[f][2q][2p] + g_f[f][2q][2p+1] + g_f[f][2q+1][2p] + g_f[f][2q+1][2p+1]) * 0.25, left to right
 *   boundary_lift:     every boundary cell c of the level: v(c) := v(c) + sign * T(c), T from phi; with phi_fine (the next finer level's phi) instead
 *                      v(c) := v(c) + sign * (T(c) - 0.125 * S(c)), S(c) = 0.0 + per face c touches (same order) the sum of the four finer
 *                      entries under its entry, summed as boundary_restrict sums them.  S is the cell restriction of the finer level's T.
 *   boundary_interp:   after interpolation_fcycle (p1) of coarse onto fine: every fine boundary cell adds D = 0.0 + weight * delta over its p1 reads
 *                      that land on a coarse ghost, in interpolation_p1's order; delta = the inhomogeneous minus the homogeneous ghost, from g_c
 *                      (the coarse level's boundary array): 2 g on a face, the linear rules of DESIGN.md §11.1 on an edge or corner.
 * g, g_c, g_f, phi, phi_fine live in the plugin's memory (hpgmg_vector_alloc).  host/hooks_host.inc holds weak host defaults (the CPU oracle); the HIP
 * plugin overrides them (kernels/dense_boundary.hip), one launch each. */
int     hpgmg_dense_pack_lifted(level_type *level, int id, const double *f, int where, const double *g, double b);
int     hpgmg_boundary_flux(level_type *level, double *phi, const double *g, double b);
void    hpgmg_boundary_restrict(level_type *coarse, double *g_c, level_type *fine, const double *g_f);
void    hpgmg_boundary_lift(level_type *level, int id, const double *phi, const double *phi_fine, double sign);
void    hpgmg_boundary_interp(level_type *fine, int id, level_type *coarse, const double *g_c);
/* Neumann and mixed walls.  mask: bit f set = domain face f (the order above) is a Neumann wall, whose entry of a boundary
 * array is the OUTWARD normal derivative gn and whose ghost is u + h gn.  The level's beta is 0.0 on a Neumann wall (the operator A_N); the
 * wall's own beta lives in `wall`, a boundary array (6 n^2; only the masked faces' entries are used), restricted with boundary_restrict.
 *   pack_walls:         hpgmg_dense_pack of a face array (same pass, same checks of every value read), except that a value on a masked domain
 *                       wall (index 0 of a box on the low wall, the high ghost layer dim of a box on the high wall) goes to `wall` and the
 *                       vector takes 0.0 there.  mask 0: hpgmg_dense_pack's bytes, `wall` untouched.
 *   pack_lifted_faces,  as pack_lifted / boundary_flux, a masked face's entry being  phi = ((b * (1.0 / h)) * wall) * gn ; the other faces
 *   flux_faces:         keep ((2.0 * b) * (1.0 / (h * h))) * beta) * g.  T(c) sums in the same order.
 *   interp_faces:       boundary_interp with the coarse iterate u_c (vector id of `coarse`) read as well.  A ghost outside along m axes, P its
 *                       cell clamped into the domain: no outside axis masked: boundary_interp's delta.  Else
 *                       delta = c * u_c(P) + s,  s = 0.0 + per outside axis in the order i, j, k (masked: h_c * gn(P), else: 2.0 * g(P)),
 *                       c = 1 - 2 * (outside axes not masked) + (m odd ? 1 : -1): the ghost u_c(P) + sum of (h_c gn | 2 (g - u_c(P))),
 *                       exact for linear u, minus the homogeneous-Dirichlet ghost (-1)^m u_c(P). */
int     hpgmg_dense_pack_walls(level_type *level, int id, const double *src, int where, int layout, int check, int mask, double *wall);
int     hpgmg_dense_pack_lifted_faces(level_type *level, int id, const double *f, int where, const double *g, double b, int mask, const double *wall);
int     hpgmg_boundary_flux_faces(level_type *level, double *phi, const double *g, double b, int mask, const double *wall);
void    hpgmg_boundary_interp_faces(level_type *fine, int id, level_type *coarse, const double *g_c, int mask);
/* Robin walls  du/dn + kappa u = g  (DESIGN.md §11.5).  A Robin wall is a masked wall like a Neumann one, with a second boundary array kappa
 * (6 n^2, >= 0, 0.0 on the faces that are not Robin; restricted with boundary_restrict) and t = kappa * h of the level.  Its ghost is
 * c u + d g, c = (2 - t) / (2 + t), d = 2 h / (2 + t): a Neumann wall is kappa = 0.0, bit for bit in everything below.
 *   check_kappa:        validates the 6 n^2 values of kappa (where: HPGMG_WHERE_*): finite everywhere, >= 0 on the faces of robin_mask.  Returns
 *                       hpgmg_dense_pack's status bits, -1 for a refused argument; *any_positive = 1 if an entry of a Robin face is > 0, else 0.
 *   store_walls:        the level's beta on the masked walls (index 0 of VECTOR_BETA_I/J/K of a box on a low wall, its high ghost layer dim on a high
 *                       wall) := wall * (t / (2.0 + t)): the homogeneous Dirichlet wall term with that beta is the Robin wall's.  rebuild_operator
 *                       (level, NULL, a, b) must follow.  kappa NULL: 0.0 everywhere.
 *   pack_lifted_robin,  pack_lifted_faces / flux_faces with a masked face's entry  phi = ((b * (1.0 / h)) * wall) * g) * (2.0 / (2.0 + t));
 *   flux_robin:         kappa NULL: the _faces forms themselves.
 *   interp_robin:       interp_faces with, per outside axis that is masked, k_a = (2.0 - t) / (2.0 + t), s_a = (2.0 * h_c / (2.0 + t)) * g(P), t from
 *                       kappa_c at P's wall entry:  delta = ((1 - (-1)^m) + sum (k_a - 1.0)) * u_c(P) + (0.0 + sum s_a), the sums in the order i, j, k,
 *                       a Dirichlet axis adding -2.0 and 2.0 * g(P).  kappa_c NULL: interp_faces itself. */
int     hpgmg_boundary_check_kappa(level_type *level, const double *kappa, int where, int robin_mask, int *any_positive);
void    hpgmg_boundary_store_walls(level_type *level, const double *wall, const double *kappa, int mask);
int     hpgmg_dense_pack_lifted_robin(level_type *level, int id, const double *f, int where, const double *g, double b, int mask, const double *wall, const double *kappa);
int     hpgmg_boundary_flux_robin(level_type *level, double *phi, const double *g, double b, int mask, const double *wall, const double *kappa);
void    hpgmg_boundary_interp_robin(level_type *fine, int id, level_type *coarse, const double *g_c, int mask, const double *kappa_c);
/* Face fluxes of vector x_id: q = -b beta du/dx_d on every face of axis d, positive towards increasing index, into three dense
 * arrays of the shapes of the beta arrays (FACE_I / J / K: one longer along their axis on a Dirichlet level, (N,N,N) on a periodic one, whose
 * face 0 lies between cell N-1 and cell 0).  With wq = b * (1.0 / h), between cells lo and hi = lo + 1:  q = (wq * beta) * (u_lo - u_hi), beta the
 * level's; on a Dirichlet wall (ghost 2 g - u_c)  q = (wq * beta) * (2.0 * (g - u_c)) low, (wq * beta) * (2.0 * (u_c - g)) high; on a masked wall
 * (mask, wall, kappa as above; t = kappa * h)  Q = ((b * wall) * (2.0 / (2.0 + t))) * (kappa * u_c - g),  q = Q high, -Q low.  Then cell by cell
 * a alpha u + (1/h) sum_d (q_d[high face] - q_d[low face])  is  A0 u - T(g).  A box writes its dim low faces along each axis and face dim where that
 * is the domain's high wall, so every entry is written once.  g, wall, kappa: boundary arrays in the plugin's memory; g NULL: zero data (required on
 * a periodic level); wall is required when mask != 0; kappa NULL: every masked wall is Neumann.  The outputs are host or plugin memory (where).  The
 * caller has filled x_id's box-to-box ghost zones (exchange_boundary); no ghost outside the domain is read.  Returns hpgmg_dense_pack's status bits
 * (HPGMG_DENSE_NOT_FINITE: an entry of g that was read is not finite), -1 for a refused argument.  Weak host default in host/hooks_host.inc; the HIP
 * plugin overrides it with one launch for the three arrays (kernels/dense_flux.hip). */
int     hpgmg_dense_unpack_flux(level_type *level, int x_id, const double *g, double b, int mask, const double *wall, const double *kappa,
                                double *flux_i, double *flux_j, double *flux_k, int where);
/* Coefficient sensitivities of a state u (vector u_id) and an adjoint lam (vector lam_id): for every coefficient entry p
 * G_p = d/dp sum_c lam_c (A0 u - T(g))_c, into d_alpha (N,N,N; NULL on a Poisson level: not written) and d_beta_i / j / k in the shapes of the beta
 * arrays (as the flux arrays above).  With w2 = b * (1.0 / (h * h)), w = (2.0 * b) * (1.0 / (h * h)), wn = b * (1.0 / h), t = kappa * h:
 *   alpha of cell c:  a * (u_c * lam_c);   between cells lo and hi = lo + 1 (the periodic wrap included):  w2 * ((u_lo - u_hi) * (lam_lo - lam_hi));
 *   a Dirichlet wall face of cell c:  (w * (u_c - g)) * lam_c;   a masked wall face:  ((wn * (2.0 / (2.0 + t))) * (kappa * u_c - g)) * lam_c
 * (include/hpgmg_boundary_math.h bnd_sens_*; either side alike).  No beta is read: a masked wall's entry is the derivative to the wall's own beta,
 * which `wall` holds; `wall` is required when mask != 0, as above, and not read.  Ownership, g, kappa, where, the refusals (-1) and the returned status
 * bits (HPGMG_DENSE_NOT_FINITE: an entry of g that was read is not finite) are hpgmg_dense_unpack_flux's.  The caller has filled the box-to-box ghost
 * zones of BOTH vectors (exchange_boundary); no ghost outside the domain is read.  Weak host default in host/hooks_host.inc; the HIP plugin overrides it
 * with one launch for the four arrays (kernels/dense_sensitivity.hip). */
int     hpgmg_dense_unpack_sensitivity(level_type *level, int u_id, int lam_id, const double *g, double a, double b, int mask, const double *wall,
                                       const double *kappa, double *d_alpha, double *d_beta_i, double *d_beta_j, double *d_beta_k, int where);
/* Cell-centred conductivities: the coefficient as ONE dense (N,N,N) array kcell, a value per cell.  The beta of a face between two
 * cells (box-to-box; the periodic wrap, lo = cell N-1 and hi = cell 0) is bnd_mean(mean, lo, hi) of include/hpgmg_boundary_math.h, lo the cell with the
 * smaller index -- harmonic (2.0 * (lo * hi)) / (lo + hi), arithmetic 0.5 * (lo + hi) -- and a domain wall face of any kind has its cell's own value.
 *   pack_cell_mean:          VECTOR_BETA_I / J / K := exactly the bytes, over every padded double of every box, that hpgmg_dense_pack (mask 0) or
 *                            hpgmg_dense_pack_walls (mask, wall) leave for those three face arrays with layouts FACE_I / J / K: under a mask `wall`
 *                            takes the masked walls' betas and the vectors 0.0 there.  Status bits: a kcell entry that is not finite NOT_FINITE, a
 *                            finite one that is not > 0 OUT_OF_RANGE; a mean is checked only when both its cells passed (lo * hi or lo + hi
 *                            overflows: NOT_FINITE; the mean underflows to zero: OUT_OF_RANGE).  After a non-zero status the vectors are
 *                            unspecified.  -1, nothing written: more than one rank, a level that is not a cube, a mask on a periodic level or
 *                            outside 0 .. 63 or without wall, kcell NULL, an unknown where or mean.
 *   unpack_cell_sensitivity: hpgmg_dense_unpack_sensitivity's d_alpha (may be NULL), and per cell c
 *                              d_k[c] = ((((G_il D_il + G_ih D_ih) + G_jl D_jl) + G_jh D_jh) + G_kl D_kl) + G_kh D_kh      (left to right)
 *                            over its six faces (low, high of i, j, k): G that pass' face sensitivity (bnd_sens_*), D the derivative of the face's
 *                            beta to k_c -- bnd_mean_dhi on a low face, bnd_mean_dlo on a high face, 1.0 on a wall.  G reads no coefficient, so the
 *                            chain rule is evaluated at the kcell handed in.  kcell is validated as the pack validates it, g as
 *                            hpgmg_dense_unpack_sensitivity does; the refusals are that hook's, and kcell or d_k NULL or an unknown mean.
 * Weak host defaults in host/hooks_host.inc (pack: the three face arrays formed with bnd_mean and packed by the existing hooks, which makes it the
 * definition; unpack: box by box); the HIP plugin overrides them with one launch each (kernels/dense_cells.hip). */
enum { HPGMG_MEAN_HARMONIC = 0, HPGMG_MEAN_ARITHMETIC = 1 };
int     hpgmg_dense_pack_cell_mean(level_type *level, const double *kcell, int where, int mean, int mask, double *wall);
int     hpgmg_dense_unpack_cell_sensitivity(level_type *level, int u_id, int lam_id, const double *kcell, int mean, const double *g, double a, double b,
                                            int mask, const double *wall, const double *kappa, double *d_alpha, double *d_k, int where);
/* The two streaming passes of the implicit time march of the user-problem API (hpgmg_user_start / hpgmg_user_step, include/hpgmg_fv.h)
 * over the interior cells of every box of a Helmholtz level (alpha = VECTOR_ALPHA); ghost and padding cells are neither read nor written:
 *   step_rhs:   F = F + ((a * alpha) * u + c * w) ;  u_old = u              (F holds f + T(g) on entry; a = 1 / (theta dt), c = (1 - theta) / theta)
 *   step_rate:  w = (r + (a * alpha) * (u - u_old)) - c * w ;  *max_abs = max |w| over the level (0.0 <= it; a NaN never becomes the maximum)
 * in exactly that written order (include/hpgmg_step_math.h, which the host defaults and the kernels both compile).  The ids are distinct vectors of
 * the level.  Weak host defaults in host/hooks_host.inc (box by box: the CPU oracle); the HIP plugin overrides them with one launch each
 * (host/plugin_step.c, kernels/dense_step.hip). */
void    hpgmg_step_rhs(level_type *level, int F_id, int u_id, int uold_id, int w_id, double a, double c);
void    hpgmg_step_rate(level_type *level, int w_id, int r_id, int u_id, int uold_id, double a, double c, double *max_abs);
/* The fine-level passes of the V-cycle-preconditioned CG of the user-problem API (MGPCGSolve, include/hpgmg_mg.h), 7-point operator:
 *   pcg_apply_dot: Ap = A p exactly as apply_op(level, Ap_id, p_id, a, b) leaves it (its ghost exchange and boundary conditions), and *dot = p . Ap
 *   pcg_update:    per interior cell  x = x + alpha * p ;  r = r - alpha * Ap  (the product first, then the sum / difference), *rmax = max |r| (0.0 <= it)
 *   pcg_dot:       *dot = a . b
 *   pcg_dot2:      *ab = a . b and *cb = c . b in one pass over the three vectors (the flexible CG's r . z and Ap . z: MGFPCGSolve);
 *                  each of the two in the order below, so *ab has the bits of pcg_dot(a, b) and *cb those of pcg_dot(c, b)
 * The two sums have ONE order, a function of the level's geometry only (it is not dot()'s): with dim the box side, the products a * b of box B are
 * formed first; column c = i + dim * j of segment s (the planes 16 s <= k < min(16 s + 16, dim)) is the chain 0.0 + q(k = 16 s) + q(16 s + 1) + ...;
 * with W = 256 * ceil(dim^2 / 256) and S = ceil(dim / 16) the chains are the leaves V[c + W * (s + S * B)] (0.0 where c >= dim^2) of an array padded
 * with 0.0 to a power of two, folded for stride = 1, 2, 4, ...:  V[m] = V[m] + V[m + stride]  for every m that is a multiple of 2 * stride; V[0] is
 * the sum.  No chain of dependent additions is longer than 16 + log2(cells).  Return value: 1 = a fused kernel of the plugin ran, 0 = the portable
 * form did (host/hooks_host.inc: the operators, then the sums on the host from downloaded boxes -- the CPU oracle; a plugin falls back to it on a level
 * its kernels do not take).  Same bits either way. */
#define HPGMG_PCG_SEGMENT 16
#define HPGMG_PCG_COLUMNS 256
int     hpgmg_pcg_apply_dot(level_type *level, int Ap_id, int p_id, double a, double b, double *dot);
int     hpgmg_pcg_update(level_type *level, int x_id, int r_id, int p_id, int Ap_id, double alpha, double *rmax);
int     hpgmg_pcg_dot(level_type *level, int a_id, int b_id, double *dot);
int     hpgmg_pcg_dot2(level_type *level, int a_id, int c_id, int b_id, double *ab, double *cb);   /* *ab = a . b, *cb = c . b */
int     hpgmg_pcg_apply_dot_host(level_type *level, int Ap_id, int p_id, double a, double b, double *dot);      /* the portable forms themselves (always 0) */
int     hpgmg_pcg_update_host(level_type *level, int x_id, int r_id, int p_id, int Ap_id, double alpha, double *rmax);
int     hpgmg_pcg_dot_host(level_type *level, int a_id, int b_id, double *dot);
int     hpgmg_pcg_dot2_host(level_type *level, int a_id, int c_id, int b_id, double *ab, double *cb);
/* Block linear algebra on one level for the eigen-solver of the user-problem API (hpgmg_user_eigs, include/hpgmg_fv.h): many inner
 * products, a linear combination of many vectors and the residuals of a block of Ritz pairs, each in ONE pass over its vectors.  All three touch
 * interior cells only: no ghost or padding double is read into a result or written.  Return value as the CG passes above (1 = the plugin's kernel ran,
 * 0 = the portable form, same bits), and -1 = refused (a count out of range, an id that is not a vector of the level, repeated outputs): nothing written.
 *   block_gram:     G[i * nb + j] = sum over the cells of w * a_i * b_j (w_id < 0: of a_i * b_j), 1 <= na, nb <= HPGMG_BLOCK_MAX_IN.  Every entry is one
 *                   tree of the CG passes' order above; its leaf term is the product a_i * b_j, weighted (w * a_i) * b_j in that association.  So an
 *                   unweighted entry has the bits of hpgmg_pcg_dot(a_i, b_j).  When the two id lists are identical, entry (i, j < i) is a copy of (j, i).
 *   block_combine:  out_j = sum_i C[i * nout + j] * in_i, 1 <= nin <= HPGMG_BLOCK_MAX_IN, 1 <= nout <= HPGMG_BLOCK_MAX_OUT: per cell the chain starts at
 *                   0.0 and runs i = 0 .. nin - 1, each product formed first.  Outputs may alias inputs (a cell reads all its inputs before it
 *                   writes); the outputs must be distinct ids.  C is a host array.
 *   block_residual: r_j = ax_j - mu_j * (w * x_j) (w_id < 0: mu_j * x_j), the product w * x first; rmax[j] = max |r_j| and mxmax[j] = max |w * x_j|
 *                   (each from 0.0; a NaN is never the maximum, as in norm()), 1 <= n <= HPGMG_BLOCK_MAX_OUT columns in one pass.  The r ids must be
 *                   distinct; r_j may be ax_j or x_j of its own column. */
#define HPGMG_BLOCK_MAX_IN 36
#define HPGMG_BLOCK_MAX_OUT 12
int     hpgmg_block_gram(level_type *level, const int *a_ids, int na, const int *b_ids, int nb, int w_id, double *G);
int     hpgmg_block_combine(level_type *level, const int *out_ids, int nout, const int *in_ids, int nin, const double *C);
int     hpgmg_block_residual(level_type *level, const int *r_ids, const int *ax_ids, const int *x_ids, int n, int w_id, const double *mu, double *rmax,
                             double *mxmax);
int     hpgmg_block_gram_host(level_type *level, const int *a_ids, int na, const int *b_ids, int nb, int w_id, double *G);      /* the portable forms themselves (0 or -1) */
int     hpgmg_block_combine_host(level_type *level, const int *out_ids, int nout, const int *in_ids, int nin, const double *C);
int     hpgmg_block_residual_host(level_type *level, const int *r_ids, const int *ax_ids, const int *x_ids, int n, int w_id, const double *mu, double *rmax,
                                  double *mxmax);
/* The three streaming passes of the Newmark march of the user-problem API (hpgmg_user_wave_start / hpgmg_user_wave_step, include/hpgmg_fv.h; DESIGN.md
 * §11.12) over the interior cells of every box of a Helmholtz level (alpha = VECTOR_ALPHA); ghost and padding doubles are neither read nor written:
 *   wave_predict:  ut = (u + dt * v) + cu * q ;  vt = v + cv * q ;  F = F + alpha * (a * ut - sigma * vt) ;  then u = ut, uold = ut, v = vt
 *                  (F holds f + T(g) on entry; cu = dt^2 (1/2 - beta), cv = dt (1 - gamma)).  5 reads, 4 writes.
 *   wave_correct:  q = (u - uold) * cq ;  v = v + cg * q  (cq = 1 / (beta dt^2), cg = gamma dt; r is the residual F - A0 u of the step's solve).
 *                  6 reads, 2 writes.
 *   wave_init:     q = ((r + (a * alpha) * u) / alpha) - sigma * v  (r = F - A0 u).  5 reads, 1 write.
 * in exactly that written order (include/hpgmg_wave_math.h, which the host defaults and the kernels both compile).  wave_correct and wave_init also
 * return sums[0] = sum over the cells of (alpha * v) * v (the new v) and sums[1] = sum of u * ((F - r) - (a * alpha) * u), each ONE tree of the CG
 * passes' order above: sums[0] has the bits of hpgmg_block_gram([v], [v], VECTOR_ALPHA).  A NaN or Inf propagates into the sums.
 * Return value as the block hooks: 1 = the plugin's kernel ran, 0 = the portable form (host/hooks_host.inc, the CPU oracle), same bits, and -1 =
 * refused (an id that is not a vector of the level, a level without alpha, a vector that is written -- u, uold, v, F of wave_predict, q and v of
 * wave_correct, q of wave_init -- named twice or equal to VECTOR_ALPHA): nothing written. */
int     hpgmg_wave_predict(level_type *level, int u_id, int uold_id, int v_id, int F_id, int q_id, double dt, double cu, double cv, double a, double sigma);
int     hpgmg_wave_correct(level_type *level, int q_id, int v_id, int u_id, int uold_id, int F_id, int r_id, double a, double cq, double cg, double sums[2]);
int     hpgmg_wave_init(level_type *level, int q_id, int r_id, int u_id, int v_id, int F_id, double a, double sigma, double sums[2]);
int     hpgmg_wave_predict_host(level_type *level, int u_id, int uold_id, int v_id, int F_id, int q_id, double dt, double cu, double cv, double a, double sigma);      /* the portable forms themselves (0 or -1) */
int     hpgmg_wave_correct_host(level_type *level, int q_id, int v_id, int u_id, int uold_id, int F_id, int r_id, double a, double cq, double cg, double sums[2]);
int     hpgmg_wave_init_host(level_type *level, int q_id, int r_id, int u_id, int v_id, int F_id, double a, double sigma, double sums[2]);
/* Launch-bound stretches of a cycle (everything done on levels of <= 64^3 cells between two
 * bottom solves) are bracketed by the cycle driver as a SEGMENT with a key that repeats every
 * solve, so the HIP plugin can capture it once into a hipGraph and replay it.  Plugins without
 * such a mechanism implement these as no-ops.  A reduction (norm/dot/mean) ends an open segment. */
void    hpgmg_segment_begin(long long key);
void    hpgmg_segment_end(void);
/* Optional fused form of MGVCycle (mg.c:1147-1163) over the chain levels[0..n-1] (finest first, levels[n-1] = bottom level).  `leg` names the part
 * (enum hpgmg_leg).  Returns 1 when the plugin executed it (bit-identical to the per-operator sequence), 0 when it cannot -- the driver then issues the
 * operators one by one. */
enum hpgmg_leg {
  HPGMG_LEG_DOWN = 0,              /* smooth, residual, restriction, zero_vector per level going down (the driver runs IterativeSolver on the bottom level afterwards) */
  HPGMG_LEG_UP = 1,                /* interpolation_vcycle, smooth per level going up */
  HPGMG_LEG_VCYCLE = 2,            /* DOWN, the bottom solve (solvers.c:27-95, BiCGStab to MG_DEFAULT_BOTTOM_NORM), UP */
  HPGMG_LEG_BOTTOM = 3,            /* the bottom solve alone (n == 1) */
  HPGMG_LEG_FCYCLE_TAIL = 4,       /* the part of FMGSolve below levels[0] (mg.c:1270-1300): restriction of R down the chain, zero_vector + bottom solve, then per
                                      level upwards interpolation_fcycle and MGVCycle, levels[0] included */
  HPGMG_LEG_FCYCLE_TAIL_ASK = 5,   /* only ask whether HPGMG_LEG_FCYCLE_TAIL would be executed (nothing runs) */
  HPGMG_LEG_FCYCLE_STEP = 6,       /* one step of FMGSolve's climb (mg.c:1289-1293): interpolation_fcycle(levels[0] <- levels[1]) and the V-cycle from levels[0] */
  HPGMG_LEG_ASK = 16               /* added to a leg: only ask whether it would be executed */
};
int     hpgmg_vcycle_legs_fused(level_type **levels, int n, int e_id, int R_id, double a, double b, int leg);
/* A plugin whose fused launches can fail AS A WHOLE (the HIP plugin's brick launches, when not all their workgroups get to run: kernels/brick_visit.hip) lets
 * the cycle driver bracket a solve it is able to repeat from its inputs: begin() = "should such a launch fail from here on, do not stop at the next scalar";
 * end() returns 1 when one did fail -- the plugin has then switched that form off, and the driver repeats the solve (host/mg.c FMGSolve).  Outside such a
 * bracket a failure stops the program with a message at the next scalar, as before.  The CPU oracle: no-ops returning 0. */
void    hpgmg_solve_attempt_begin(void);
int     hpgmg_solve_attempt_end(void);
/* The whole bottom solve -- IterativeSolver's BiCGStab (solvers/bicgstab.c:14-97) on level L: e_id = initial guess and solution -- as one device
 * launch where the plugin has one (27-point / fv2 / fv4: a bottom level of one small box, Dirichlet); 0 = not taken, the caller runs the
 * host-driven solver.  Same iterates, same iteration count (folded into L->Krylov_iterations by hpgmg_level_sync_counters). */
int     hpgmg_bottom_solve_fused(level_type *L, int e_id, int R_id, double a, double b, double desired_reduction_in_norm);
/* Optional fused form of  interpolation_vcycle(fine, e, 1.0, coarse, e); smooth(fine, e, R)  (mg.c:1160-1161): returns 1 when the
 * plugin executed both (same iterate; VECTOR_TEMP unspecified, as with hpgmg_smooth_in_cycle), 0 when the driver must call the two operators. */
int     hpgmg_interp_smooth_fused(level_type *fine, int e_id, int R_id, level_type *coarse, double a, double b);
/* Optional fused form of  restriction(coarse, id_c, fine, id_f, RESTRICT_CELL); zero_vector(coarse, zero_id)  (mg.c:1152-1153) */
int     hpgmg_restrict_zero_fused(level_type *coarse, int id_c, level_type *fine, int id_f, int zero_id);
/* Timing hooks for the cycle driver's per-level "Total" rows (mg.c:54-161).  The plugin decides what a tick measures: the
 * CPU oracle reads the host clock; the HIP plugin, whose launches are asynchronous, can record a hipEvent pair instead and
 * add the elapsed DEVICE time to *acc later -- hpgmg_timers_settle() (also done by hpgmg_level_sync_counters) makes every
 * pending tick land in its accumulator.  `what` names the range for profilers (roctx). */
typedef struct { double t0; double *acc; int slot, range; } hpgmg_tick;
hpgmg_tick hpgmg_tick_begin(level_type *level, double *acc_seconds, const char *what);
void    hpgmg_tick_end(hpgmg_tick t);
void    hpgmg_timers_settle(void);
/* 0 host clock around (asynchronous) operator calls, 1 device time per operator (hipEvent pairs), 2 synchronise around every
 * operator; the CPU oracle ignores it.  Environment: HPGMG_TIMERS=host|device|sync. */
void    hpgmg_set_timer_mode(int mode);
int     hpgmg_get_timer_mode(void);
/* Optional fused forms around residual() (return 1 when executed, 0 when the driver must issue the operators one by one):
 *   residual(fine, TEMP, x, rhs); restriction(coarse, id_c, fine, TEMP, RESTRICT_CELL); zero_vector(coarse, zero_id)   (mg.c:1150-1153)
 *     -- same coarse result; the fine level's VECTOR_TEMP is left untouched (the residual is never stored);
 *   residual(level, res, x, rhs); *norm_out = norm(level, res)                                                          (mg.c:1321-1323)
 *     -- res_id < 0: only the norm is wanted (the cycle driver's convergence check: nothing reads the residual afterwards) */
int     hpgmg_residual_restrict_zero_fused(level_type *coarse, int id_c, level_type *fine, int x_id, int rhs_id, double a, double b, int zero_id);
int     hpgmg_residual_norm_fused(level_type *level, int res_id, int x_id, int rhs_id, double a, double b, double *norm_out);
/*   *norm_out = norm(level, F); scale_vector(level, R, 1.0, F); restriction(coarse, R, level, R, RESTRICT_CELL)                        (mg.c:1262-1270) */
int     hpgmg_norm_scale_restrict_fused(level_type *level, int F_id, int R_id, level_type *coarse, double *norm_out);
/*   the same with the norm collected LATER by hpgmg_norm_deferred_fetch(level) (once, before anything else defers): FMGSolve uses norm(F) only in the check at its end */
int     hpgmg_norm_scale_restrict_fused_deferred(level_type *level, int F_id, int R_id, level_type *coarse);
double  hpgmg_norm_deferred_fetch(level_type *level);
/*   zero_vector(fine, id_f); interpolation_fcycle(fine, id_f, 0.0, coarse, id_c) -- the benchmark step's zero_vector(u) (hpgmg-fv.c:77-85) and the F-cycle's
 *   first write of u on that level (mg.c:1295) -- as one launch: same interior; the ghost zones zero_vector would clear may keep their content */
int     hpgmg_zero_interpolation_fcycle_fused(level_type *fine, int id_f, level_type *coarse, int id_c);
/* smooth() for callers to whom VECTOR_TEMP is scratch afterwards (MGVCycle: the operator that follows a smooth() overwrites or ignores
 * it): same iterate in phi_id, VECTOR_TEMP unspecified.  Returns 1 when executed, 0 when the caller must call smooth(). */
int     hpgmg_smooth_in_cycle(level_type *level, int phi_id, int rhs_id, double a, double b);
/* The operators that return nothing may be postponed by a plugin: the HIP plugin records smooth / residual / restriction / zero_vector /
 * interpolation_vcycle while they follow the order MGVCycle issues them in (mg.c:1145-1164) and runs them, fused where it can, at the first
 * call that does not -- so the reference's unmodified driver gets the fused forms too (INTEGRATION.md Route B).  The state every later call
 * sees is exactly the one the separate operators leave.  hpgmg_operators_flush() issues what is pending (tests that count launches use it),
 * hpgmg_set_lazy(0) / HPGMG_LAZY=0 turns the queue off.  The CPU oracle implements both as no-ops. */
void    hpgmg_operators_flush(void);
void    hpgmg_set_lazy(int on);
/* bring level->Krylov_iterations up to date with bottom solves the plugin ran asynchronously */
void    hpgmg_level_sync_counters(level_type *level);
/* called by destroy_level / MGDestroy so the plugin can drop device mirrors */
void    hpgmg_level_release(level_type *level);
const char *hpgmg_backend_name(void);                      /* "hip" or "oracle-cpu" */

#ifdef __cplusplus
}
#endif
#endif
