/*
 * solvers.c -- bottom (coarsest level) solver: diagonally preconditioned
 * BiCGStab (default) or CG, or the s-step CABiCGStab / CACG, driven from the
 * host through operators.h (and, for the s-step ones, matmul) only.
 *
 * Behavioural reference: finite-volume/source/solvers.c:27-95 and
 * solvers/bicgstab.c:14-97 (Saad, Iterative Methods, Alg. 7.7 with a right
 * preconditioner M = D).  The sequence of operator calls and the break-down
 * tests are the same, because the number of bottom iterations per solve and
 * the coarse correction they produce feed the pinned F-cycle norms.
 * north_star: "BiCGStab on the coarse bottom stays on host" -- the control flow
 * and every scalar live here; vectors stay wherever the plugin keeps them.
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <time.h>
#include "hpgmg_level.h"
#include "hpgmg_operators.h"
#include "hpgmg_mg.h"

#define CA_KRYLOV_S 4   /* cabicgstab.c:17-19, cacg.c:12-14 */

/* BiCGStab: r0, r, p, q, s, t, Ap, As; CG: r0, r, p, Ap, z; CABiCGStab: rt, r, p, P[2s+1], R[2s], and r tilde's slot; CACG: r0, r, p, P[s+1], R[s]
 * (solvers.c:92-104) */
int IterativeSolver_NumVectors(void) {
  switch (hpgmg_get_bottom_solver()) {
    case HPGMG_BOTTOM_CG:         return 5;
    case HPGMG_BOTTOM_CABICGSTAB: return 4 + 4 * CA_KRYLOV_S;
    case HPGMG_BOTTOM_CACG:       return 4 + 2 * CA_KRYLOV_S;
    default:                      return 8;
  }
}

static double now(void) { struct timespec t; clock_gettime(CLOCK_MONOTONIC, &t); return (double)t.tv_sec + 1e-9 * (double)t.tv_nsec; }

static void remove_mean(level_type *L, int id) {
  if (L->must_subtract_mean == 1) {
    double m = mean(L, id);
    shift_vector(L, id, id, -m);
  }
}

/* the s-step solvers' small dense helpers (cabicgstab.c:23-45, cacg.c:18-40), same arithmetic in the same order.  gemv: z = alpha A x + beta y,
 * A row-major with leading dimension lda; z may be y. */
static void gemv(double *z, double alpha, const double *A, int lda, const double *x, double beta, const double *y, int rows, int cols) {
  int r, c;
  for (r = 0; r < rows; r++) {
    double sum = 0.0;
    for (c = 0; c < cols; c++) sum += A[r * lda + c] * x[c];
    z[r] = alpha * sum + beta * y[r];
  }
}
static void axpy(double *z, double alpha, const double *x, double beta, const double *y, int n) { int i; for (i = 0; i < n; i++) z[i] = alpha * x[i] + beta * y[i]; }
static double vdotv(const double *x, const double *y, int n) { int i; double sum = 0.0; for (i = 0; i < n; i++) sum += x[i] * y[i]; return sum; }
static void zero(double *z, int n) { int i; for (i = 0; i < n; i++) z[i] = 0.0; }

/* matmul's ONE reduction (matmul.c:49-59, MPI_Allreduce of the whole matrix): through the transport over the level's active ranks, which add the
 * ranks' matrices in rank order as dot() does */
static void matmul_allreduce(level_type *L, double *C, int n) {
  const hpgmg_transport *T = hpgmg_get_transport();
  if (T && T->size > 1) {
    hpgmg_level_ext *X = hpgmg_level_ext_get(L);
    if (X->num_active_ranks > 1) {
      const double t0 = now();
      T->allreduce(T->ctx, C, n, HPGMG_REDUCE_SUM, X->active_ranks, X->num_active_ranks);
      L->timers.collectives += now() - t0;
    }
  }
}

static void bicgstab(level_type *L, int x_id, int R_id, double a, double b, double want) {
  const int base = hpgmg_vectors_reserved();
  const int r0 = base + 0, r = base + 1, p = base + 2, q = base + 3, s = base + 4, t = base + 5, Ap = base + 6, As = base + 7;
  const int max_iters = 200;
  int it = 0;

  residual(L, r0, x_id, R_id, a, b);
  remove_mean(L, r0);
  scale_vector(L, r, 1.0, r0);
  scale_vector(L, p, 1.0, r0);
  double rho = dot(L, r, r0);
  const double r0_norm = norm(L, r);
  if (rho == 0.0 || r0_norm == 0.0) return; /* entered with the exact solution */

  while (it < max_iters) {
    it++;
    L->Krylov_iterations++;
    mul_vectors(L, q, 1.0, VECTOR_DINV, p);              /* q = M^-1 p */
    apply_op(L, Ap, q, a, b);
    double Ap_r0 = dot(L, Ap, r0);
    if (Ap_r0 == 0.0) break;                              /* pivot breakdown */
    double alpha = rho / Ap_r0;
    if (isinf(alpha)) break;
    add_vectors(L, x_id, 1.0, x_id, alpha, q);
    add_vectors(L, s, 1.0, r, -alpha, Ap);                /* s = r - alpha A q */
    remove_mean(L, s);
    double s_norm = norm(L, s);
    if (s_norm == 0.0 || s_norm < want * r0_norm) break;  /* converged on the half step */
    mul_vectors(L, t, 1.0, VECTOR_DINV, s);              /* t = M^-1 s */
    apply_op(L, As, t, a, b);
    double As_As = dot(L, As, As);
    double As_s  = dot(L, As, s);
    if (As_As == 0.0) break;
    double omega = As_s / As_As;
    if (omega == 0.0 || isinf(omega)) break;              /* stabilisation breakdown */
    add_vectors(L, x_id, 1.0, x_id, omega, t);
    add_vectors(L, r, 1.0, s, -omega, As);
    remove_mean(L, r);
    double r_norm = norm(L, r);
    if (r_norm == 0.0 || r_norm < want * r0_norm) break;
    double rho_new = dot(L, r, r0);
    if (rho_new == 0.0) break;                            /* Lanczos breakdown */
    double beta = (rho_new / rho) * (alpha / omega);
    if (isinf(beta)) break;
    add_vectors(L, VECTOR_TEMP, 1.0, p, -omega, Ap);
    add_vectors(L, p, 1.0, r, beta, VECTOR_TEMP);         /* p = r + beta (p - omega Ap) */
    rho = rho_new;
  }
}

/* The reference's other host-driven choice, -DUSE_CG (solvers/cg.c:14-77; Saad, algorithm 9.1 with the diagonal as preconditioner): same calls,
 * same order, same break-down tests -- the iteration count and the correction feed the pinned norms exactly as BiCGStab's do. */
static void cg(level_type *L, int x_id, int R_id, double a, double b, double want) {
  const int base = hpgmg_vectors_reserved();
  const int r0 = base + 0, r = base + 1, p = base + 2, Ap = base + 3, z = base + 4;
  const int max_iters = 200;
  int it = 0;
  residual(L, r0, x_id, R_id, a, b);
  remove_mean(L, r0);
  scale_vector(L, r, 1.0, r0);
  mul_vectors(L, z, 1.0, VECTOR_DINV, r0);               /* z = D^-1 r0 */
  scale_vector(L, p, 1.0, z);
  const double r0_norm = norm(L, r);
  if (r0_norm == 0.0) return;                             /* entered with the exact solution */
  double r_dot_z = dot(L, r, z);
  while (it < max_iters) {
    it++;
    L->Krylov_iterations++;
    apply_op(L, Ap, p, a, b);
    const double Ap_p = dot(L, Ap, p);
    if (Ap_p == 0.0) break;                               /* pivot breakdown */
    const double alpha = r_dot_z / Ap_p;
    if (isinf(alpha)) break;
    add_vectors(L, x_id, 1.0, x_id, alpha, p);
    add_vectors(L, r, 1.0, r, -alpha, Ap);
    remove_mean(L, r);
    const double r_norm = norm(L, r);
    if (r_norm == 0.0 || r_norm < want * r0_norm) break;
    mul_vectors(L, z, 1.0, VECTOR_DINV, r);
    const double r_dot_z_new = dot(L, r, z);
    if (r_dot_z_new == 0.0) break;                        /* Lanczos breakdown */
    const double beta = r_dot_z_new / r_dot_z;
    if (isinf(beta)) break;
    add_vectors(L, p, 1.0, z, beta, p);
    r_dot_z = r_dot_z_new;
  }
}

/* ---- the s-step solvers' Gram matrix: solvers/matmul.c:6-62 --------------------------------------------------------------------------------
 * The default: every box of every vector it names is downloaded once (hpgmg_vector_download) and each upper-triangle entry formed on the host in
 * the reference's order -- a chain over the box's interior in k, j, i order per box, the box partials added in box order.  Weak, so that a plugin
 * that forms the matrix itself (the HIP plugin: one Gram launch) replaces it, while a plugin without one (the CPU oracle) gets this. */
__attribute__((weak)) void matmul(level_type *L, double *C, int *id_A, int *id_B, int rows, int cols, int A_equals_B_transpose) {
  const double t0 = now();
  int mm, nn, box, v;
  int ids[128], nids = 0, slot_A[64], slot_B[64];
  (void)A_equals_B_transpose;
  if (rows < 1 || cols < 1 || rows > 64 || cols > 64) { fprintf(stderr, "matmul: %d x %d is outside 1..64 x 1..64\n", rows, cols); abort(); }
  for (v = 0; v < rows + cols; v++) {      /* each vector downloaded once per box */
    const int id = v < rows ? id_A[v] : id_B[v - rows];
    int q;
    for (q = 0; q < nids && ids[q] != id; q++) {}
    if (q == nids) ids[nids++] = id;
    if (v < rows) slot_A[v] = q; else slot_B[v - rows] = q;
  }
  for (mm = 0; mm < rows * cols; mm++) C[mm] = 0.0;
  double *level_sum = (double *)calloc((size_t)rows * cols, sizeof(double));
  double *host = (double *)malloc((size_t)nids * (L->num_my_boxes > 0 ? L->my_boxes[0].volume : 1) * sizeof(double));
  for (box = 0; box < L->num_my_boxes; box++) {
    const box_type *B = &L->my_boxes[box];
    const int jS = B->jStride, kS = B->kStride, g = B->ghosts, dim = B->dim, origin = g * (1 + jS + kS);
    for (v = 0; v < nids; v++) hpgmg_vector_download(host + (size_t)v * B->volume, B->vectors[ids[v]], (size_t)B->volume);
    for (mm = 0; mm < rows; mm++) for (nn = mm; nn < cols; nn++) {       /* upper triangle, matmul.c:33 */
      const double *a = host + (size_t)slot_A[mm] * B->volume + origin, *b = host + (size_t)slot_B[nn] * B->volume + origin;
      double box_sum = 0.0;
      int i, j, k;
      for (k = 0; k < dim; k++) for (j = 0; j < dim; j++) for (i = 0; i < dim; i++) { const int ijk = i + j * jS + k * kS; box_sum += a[ijk] * b[ijk]; }
      level_sum[mm * cols + nn] += box_sum;
    }
  }
  for (mm = 0; mm < rows; mm++) for (nn = mm; nn < cols; nn++) {
    C[mm * cols + nn] = level_sum[mm * cols + nn];
    if (mm < cols && nn < rows) C[nn * cols + mm] = level_sum[mm * cols + nn];      /* matmul.c:45-46 */
  }
  free(host); free(level_sum);
  L->timers.blas3 += now() - t0;
  matmul_allreduce(L, C, rows * cols);
}

/* -DUSE_CABICGSTAB: solvers/cabicgstab.c:49-283, the telescoping form (s = 1, 2, 4, 4, ...) the reference compiles by default; Carson, Demmel and
 * Knight's s-step BiCGStab with the monomial basis.  Same operator calls in the same order, the same small dense arithmetic in the same order,
 * the same exit tests: the iteration count and the correction feed the pinned norms. */
#define CA_N (4 * CA_KRYLOV_S + 1)
static void cabicgstab(level_type *L, int x_id, int R_id, double a, double b, double want) {
  const int base = hpgmg_vectors_reserved();
  const int rt = base + 0, r = base + 1, p = base + 2, PRrt_id = base + 3;
  double temp1[CA_N], temp2[CA_N], temp3[CA_N], Tp[CA_N][CA_N], Tpp[CA_N][CA_N], aj[CA_N], cj[CA_N], ej[CA_N], Tpaj[CA_N], Tpcj[CA_N], Tppaj[CA_N];
  double G[CA_N][CA_N], g[CA_N], Gg[CA_N * (CA_N + 1)];
  int PRrt[CA_N + 1];
  const int max_iters = 200;
  int m = 0, n, i, j, k, failed = 0, converged = 0;
  double alpha, omega, delta, beta;

  residual(L, rt, x_id, R_id, a, b);
  scale_vector(L, r, 1.0, rt);
  scale_vector(L, p, 1.0, rt);
  const double rt_norm = norm(L, rt);
  if (rt_norm == 0.0) converged = 1;                                      /* entered with the exact solution */
  delta = dot(L, r, rt);
  if (delta == 0.0) converged = 1;
  const double rt_l2 = sqrt(delta);

  int s = 1;                                                               /* telescoping: s = 1, 2, 4, 4, ... (cabicgstab.c:99, :276) */
  while (m < max_iters && !failed && !converged) {
    const int ns = 4 * s + 1;
    zero(aj, ns); zero(cj, ns); zero(ej, ns); zero(Tpaj, ns); zero(Tpcj, ns); zero(Tppaj, ns); zero(temp1, ns); zero(temp2, ns); zero(temp3, ns);
    for (i = 0; i < ns; i++) for (j = 0; j < ns; j++) Tp[i][j] = 0;
    for (i = 0; i < ns; i++) for (j = 0; j < ns; j++) Tpp[i][j] = 0;
    for (i = 0; i < 2 * s; i++) Tp[i + 1][i] = 1;                         /* monomial basis (cabicgstab.c:114-117) */
    for (i = 2 * s + 1; i < 4 * s; i++) Tp[i + 1][i] = 1;
    for (i = 0; i < 2 * s - 1; i++) Tpp[i + 2][i] = 1;
    for (i = 2 * s + 1; i < 4 * s - 1; i++) Tpp[i + 2][i] = 1;
    for (i = 0; i < ns; i++) PRrt[i] = PRrt_id + i;
    PRrt[ns] = rt;
    const int *P = PRrt, *Rp = PRrt + 2 * s + 1;                          /* P[n] = A^n p (2s + 1 of them), Rp[n] = A^n r (2s) */

    scale_vector(L, P[0], 1.0, p);
    for (n = 1; n < 2 * s + 1; n++) apply_op(L, P[n], P[n - 1], a, b);
    scale_vector(L, Rp[0], 1.0, r);
    for (n = 1; n < 2 * s; n++) apply_op(L, Rp[n], Rp[n - 1], a, b);

    L->CAKrylov_formations_of_G++;
    matmul(L, Gg, PRrt, PRrt, ns, ns + 1, 1);                             /* [P,R]^T [P,R,rt] */
    for (i = 0, k = 0; i < ns; i++) {
      for (j = 0; j < ns; j++) G[i][j] = Gg[k++];
      g[i] = Gg[k++];
    }
    for (i = 0; i < ns; i++) aj[i] = 0.0;
    aj[0] = 1.0;
    for (i = 0; i < ns; i++) cj[i] = 0.0;
    cj[2 * s + 1] = 1.0;
    for (i = 0; i < ns; i++) ej[i] = 0.0;

    for (n = 0; n < s; n++) {
      L->Krylov_iterations++;
      gemv(Tpaj, 1.0, &Tp[0][0], CA_N, aj, 0.0, Tpaj, ns, ns);
      gemv(Tpcj, 1.0, &Tp[0][0], CA_N, cj, 0.0, Tpcj, ns, ns);
      gemv(Tppaj, 1.0, &Tpp[0][0], CA_N, aj, 0.0, Tppaj, ns, ns);
      const double g_dot_Tpaj = vdotv(g, Tpaj, ns);
      if (g_dot_Tpaj == 0.0) { failed = 1; break; }                       /* pivot breakdown */
      alpha = delta / g_dot_Tpaj;
      if (isinf(alpha)) { failed = 1; break; }
      axpy(temp1, 1.0, Tpcj, -alpha, Tppaj, ns);                          /* the #else form of cabicgstab.c:184-189: G applied to the difference */
      gemv(temp2, 1.0, &G[0][0], CA_N, temp1, 0.0, temp2, ns, ns);
      axpy(temp3, 1.0, cj, -alpha, Tpaj, ns);
      const double omega_num = vdotv(temp3, temp2, ns);
      const double omega_den = vdotv(temp1, temp2, ns);
      axpy(ej, 1.0, ej, alpha, aj, ns);                                   /* the partial update comes before the omega test (cabicgstab.c:195-196) */
      axpy(temp1, 1.0, cj, -alpha, Tpaj, ns);
      gemv(temp2, 1.0, &G[0][0], CA_N, temp1, 0.0, temp2, ns, ns);
      double s_l2 = vdotv(temp1, temp2, ns);                              /* ||s||^2 in exact arithmetic; flushed to 0 when negative */
      if (s_l2 < 0) s_l2 = 0; else s_l2 = sqrt(s_l2);
      if (s_l2 < want * rt_l2) { converged = 1; break; }
      if (omega_den == 0.0) { failed = 1; break; }
      omega = omega_num / omega_den;
      if (isinf(omega)) { failed = 1; break; }
      axpy(ej, 1.0, ej, omega, cj, ns);
      axpy(ej, 1.0, ej, -omega * alpha, Tpaj, ns);
      axpy(cj, 1.0, cj, -omega, Tpcj, ns);
      axpy(cj, 1.0, cj, -alpha, Tpaj, ns);
      axpy(cj, 1.0, cj, omega * alpha, Tppaj, ns);
      gemv(temp1, 1.0, &G[0][0], CA_N, cj, 0.0, temp1, ns, ns);
      const double cj_dot_Gcj = vdotv(cj, temp1, ns);
      double r_l2 = 0.0;
      if (cj_dot_Gcj > 0) r_l2 = sqrt(cj_dot_Gcj);
      if (r_l2 < want * rt_l2) { converged = 1; break; }
      const double delta_next = vdotv(g, cj, ns);
      if (isinf(delta_next)) { failed = 1; break; }
      if (delta_next == 0.0) { failed = 1; break; }                       /* Lanczos breakdown */
      if (omega == 0.0) { failed = 1; break; }                            /* stabilisation breakdown */
      beta = (delta_next / delta) * (alpha / omega);
      if (isinf(beta)) { failed = 1; break; }
      if (beta == 0.0) { failed = 1; break; }
      axpy(aj, 1.0, cj, beta, aj, ns);
      axpy(aj, 1.0, aj, -omega * beta, Tpaj, ns);
      delta = delta_next;
    }

    for (i = 0; i < ns; i++) add_vectors(L, x_id, 1.0, x_id, ej[i], PRrt[i]);      /* x += [P,R] ej */
    if (!failed && !converged) {
      add_vectors(L, p, 0.0, p, aj[0], PRrt[0]);                                    /* p = [P,R] aj */
      for (i = 1; i < ns; i++) add_vectors(L, p, 1.0, p, aj[i], PRrt[i]);
      add_vectors(L, r, 0.0, r, cj[0], PRrt[0]);                                    /* r = [P,R] cj */
      for (i = 1; i < ns; i++) add_vectors(L, r, 1.0, r, cj[i], PRrt[i]);
    }
    m += s;
    s *= 2;
    if (s > CA_KRYLOV_S) s = CA_KRYLOV_S;
  }
}
#undef CA_N

/* -DUSE_CACG: solvers/cacg.c:44-169 (s-step CG with the monomial basis, s = CA_KRYLOV_S throughout), restated like cabicgstab() above */
#define CA_N (2 * CA_KRYLOV_S + 1)
static void cacg(level_type *L, int x_id, int R_id, double a, double b, double want) {
  const int base = hpgmg_vectors_reserved();
  const int r0 = base + 0, r = base + 1, p = base + 2, PR_id = base + 3;
  double temp1[CA_N], temp2[CA_N], temp3[CA_N], aj[CA_N], cj[CA_N], ej[CA_N], Tpaj[CA_N], Tp[CA_N][CA_N], G[CA_N][CA_N], Gbuf[CA_N * CA_N];
  int PR[CA_N];
  const int *P = PR, *Rp = PR + CA_KRYLOV_S + 1;                          /* P[n] = A^n p (s + 1 of them), Rp[n] = A^n r (s) */
  const int max_iters = 200;
  int m = 0, n, i, j, k, failed = 0, converged = 0;
  double alpha, beta;

  residual(L, r0, x_id, R_id, a, b);
  scale_vector(L, r, 1.0, r0);
  scale_vector(L, p, 1.0, r0);
  const double r0_norm = norm(L, r0);
  if (r0_norm == 0.0) converged = 1;                                      /* entered with the exact solution */
  const double delta = dot(L, r, r0);
  if (delta == 0.0) converged = 1;
  const double r0_l2 = sqrt(delta);

  for (i = 0; i < CA_N; i++) for (j = 0; j < CA_N; j++) Tp[i][j] = 0;
  for (i = 0; i < CA_KRYLOV_S; i++) Tp[i + 1][i] = 1;                     /* monomial basis (cacg.c:86-88) */
  for (i = CA_KRYLOV_S + 1; i < 2 * CA_KRYLOV_S; i++) Tp[i + 1][i] = 1;
  for (i = 0; i < CA_N; i++) PR[i] = PR_id + i;

  while (m < max_iters && !failed && !converged) {
    zero(aj, CA_N); zero(cj, CA_N); zero(ej, CA_N); zero(Tpaj, CA_N); zero(temp1, CA_N); zero(temp2, CA_N); zero(temp3, CA_N);
    scale_vector(L, P[0], 1.0, p);
    for (n = 1; n < CA_KRYLOV_S + 1; n++) apply_op(L, P[n], P[n - 1], a, b);
    scale_vector(L, Rp[0], 1.0, r);
    for (n = 1; n < CA_KRYLOV_S; n++) apply_op(L, Rp[n], Rp[n - 1], a, b);

    L->CAKrylov_formations_of_G++;
    matmul(L, Gbuf, PR, PR, CA_N, CA_N, 1);                                /* [P,R]^T [P,R] */
    for (i = 0, k = 0; i < CA_N; i++) for (j = 0; j < CA_N; j++) G[i][j] = Gbuf[k++];
    for (i = 0; i < CA_N; i++) aj[i] = 0.0;
    aj[0] = 1.0;
    for (i = 0; i < CA_N; i++) cj[i] = 0.0;
    cj[CA_KRYLOV_S + 1] = 1.0;
    for (i = 0; i < CA_N; i++) ej[i] = 0.0;

    for (n = 0; n < CA_KRYLOV_S; n++) {
      L->Krylov_iterations++;
      gemv(Tpaj, 1.0, &Tp[0][0], CA_N, aj, 0.0, Tpaj, CA_N, CA_N);
      gemv(temp1, 1.0, &G[0][0], CA_N, Tpaj, 0.0, temp1, CA_N, CA_N);
      gemv(temp2, 1.0, &G[0][0], CA_N, cj, 0.0, temp2, CA_N, CA_N);
      const double aj_dot_GTpaj = vdotv(aj, temp1, CA_N);
      const double cj_dot_Gcj = vdotv(cj, temp2, CA_N);
      if (aj_dot_GTpaj == 0.0) { failed = 1; break; }                     /* pivot breakdown */
      alpha = cj_dot_Gcj / aj_dot_GTpaj;
      if (isinf(alpha)) { failed = 1; break; }
      axpy(ej, 1.0, ej, alpha, aj, CA_N);
      axpy(cj, 1.0, cj, -alpha, Tpaj, CA_N);
      gemv(temp2, 1.0, &G[0][0], CA_N, cj, 0.0, temp2, CA_N, CA_N);
      const double cj_dot_Gcj_new = vdotv(cj, temp2, CA_N);
      double r_l2 = 0.0;
      if (cj_dot_Gcj_new > 0) r_l2 = sqrt(cj_dot_Gcj_new);                /* flushed to 0 when negative */
      if (r_l2 < want * r0_l2) { converged = 1; break; }
      if (cj_dot_Gcj_new == 0.0) { failed = 1; break; }                   /* Lanczos breakdown */
      beta = cj_dot_Gcj_new / cj_dot_Gcj;
      if (isinf(beta)) { failed = 1; break; }
      if (beta == 0.0) { failed = 1; break; }
      axpy(aj, 1.0, cj, beta, aj, CA_N);
    }

    for (i = 0; i < CA_N; i++) add_vectors(L, x_id, 1.0, x_id, ej[i], PR[i]);      /* x += [P,R] ej */
    if (!failed && !converged) {
      add_vectors(L, p, 0.0, p, aj[0], PR[0]);                                      /* p = [P,R] aj */
      for (i = 1; i < CA_N; i++) add_vectors(L, p, 1.0, p, aj[i], PR[i]);
      add_vectors(L, r, 0.0, r, cj[0], PR[0]);                                      /* r = [P,R] cj */
      for (i = 1; i < CA_N; i++) add_vectors(L, r, 1.0, r, cj[i], PR[i]);
    }
    m += CA_KRYLOV_S;
  }
}
#undef CA_N

void IterativeSolver(level_type *L, int u_id, int f_id, double a, double b, double desired_reduction_in_norm) {
  if (!L->active) return;
  if (L->must_subtract_mean == -1) {
    int alpha_is_zero = 1;
    L->must_subtract_mean = 0;
    if (hpgmg_vectors_reserved() > VECTOR_ALPHA) alpha_is_zero = (dot(L, VECTOR_ALPHA, VECTOR_ALPHA) == 0.0);
    if (L->boundary_condition.type == BC_PERIODIC && (a == 0 || alpha_is_zero)) L->must_subtract_mean = 1;
  }
  if (hpgmg_get_bottom_solver() == HPGMG_BOTTOM_CG) { cg(L, u_id, f_id, a, b, desired_reduction_in_norm); return; }
  if (hpgmg_get_bottom_solver() == HPGMG_BOTTOM_CABICGSTAB) { cabicgstab(L, u_id, f_id, a, b, desired_reduction_in_norm); return; }
  if (hpgmg_get_bottom_solver() == HPGMG_BOTTOM_CACG) { cacg(L, u_id, f_id, a, b, desired_reduction_in_norm); return; }
  if (L->must_subtract_mean != 1 && hpgmg_bottom_solve_fused(L, u_id, f_id, a, b, desired_reduction_in_norm)) return;   /* the same solver as one device launch */
  bicgstab(L, u_id, f_id, a, b, desired_reduction_in_norm);
}
