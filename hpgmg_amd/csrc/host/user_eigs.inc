/*
 * user_eigs.inc -- hpgmg_user_eigs (include/hpgmg_fv.h): the lowest eigenmodes of a user problem by LOBPCG around the V-cycle (DESIGN.md §11.11).
 * The fine-level work is the three block hooks of include/hpgmg_operators.h (host defaults: host/hooks_host.inc; HIP: host/plugin_block.c), apply_op and
 * one V-cycle per active column; the Rayleigh-Ritz step is plain C on matrices of at most 36 x 36.  A part of host/driver.c's translation unit, included
 * there after user_solver.inc.
 */
#define EIG_M HPGMG_USER_EIGS_MAX_BLOCK
#define EIG_S (3 * EIG_M)              /* the most columns of S = [X, W, P] */
#define EIG_PIVOT_MIN 1.0e-13          /* Cholesky of the unit-diagonal Gram matrix: a pivot at or below this is a dependent basis */
#define EIG_REFRESH 10                 /* A X is applied afresh every so many iterations */

/* The generalised symmetric problem GA c = theta GM c of order n on the host: GA is symmetrised, both are scaled to a unit diagonal of GM, GM = L L^T,
 * cyclic Jacobi on L^-1 GA L^-T; the `take` lowest pairs: theta ascending and C (n x take, row-major) = D L^-T Q with C^T GM C = I.  Returns 0, or -1 when
 * GM is not positive definite to EIG_PIVOT_MIN or a value is not finite (C and theta are then untouched).  GA and GM are destroyed.  The matrices live in
 * a workspace the call owns (about 150 KB, from the heap): two solvers on two threads do not meet in it. */
typedef struct {
  double Lc[EIG_S][EIG_S], B[EIG_S][EIG_S], Q[EIG_S][EIG_S];                                                        /* eig_ritz's */
  double GA[EIG_S * EIG_S], GM[EIG_S * EIG_S], GA0[EIG_S * EIG_S], GM0[EIG_S * EIG_S], C[EIG_S * EIG_M], C2[EIG_S * EIG_M];      /* hpgmg_user_eigs' */
} eig_work;
static int eig_ritz(eig_work *work, int n, double *GA, double *GM, int take, double *C, double *theta) {
  double (*Lc)[EIG_S] = work->Lc, (*B)[EIG_S] = work->B, (*Q)[EIG_S] = work->Q;
  double d[EIG_S], y[EIG_S];
  int order[EIG_S], i, j, k, sweep;
  for (i = 0; i < n; i++) {
    const double g = GM[i * n + i];
    if (!(g > 0.0) || !isfinite(g)) return -1;
    d[i] = 1.0 / sqrt(g);
  }
  for (i = 0; i < n; i++) for (j = i; j < n; j++) {
    const double ga = 0.5 * (GA[i * n + j] + GA[j * n + i]), gm = GM[i * n + j];
    if (!isfinite(ga) || !isfinite(gm)) return -1;
    GA[i * n + j] = GA[j * n + i] = d[i] * ga * d[j];
    GM[i * n + j] = GM[j * n + i] = d[i] * gm * d[j];
  }
  for (j = 0; j < n; j++) {                                        /* GM = L L^T */
    double sum = GM[j * n + j];
    for (k = 0; k < j; k++) sum -= Lc[j][k] * Lc[j][k];
    if (!(sum > EIG_PIVOT_MIN)) return -1;
    Lc[j][j] = sqrt(sum);
    for (i = j + 1; i < n; i++) {
      double t = GM[i * n + j];
      for (k = 0; k < j; k++) t -= Lc[i][k] * Lc[j][k];
      Lc[i][j] = t / Lc[j][j];
    }
  }
  for (j = 0; j < n; j++)                                          /* B = L^-1 GA: forward substitution, column by column */
    for (i = 0; i < n; i++) {
      double t = GA[i * n + j];
      for (k = 0; k < i; k++) t -= Lc[i][k] * B[k][j];
      B[i][j] = t / Lc[i][i];
    }
  for (i = 0; i < n; i++)                                          /* B = B L^-T: the same on its rows */
    for (j = 0; j < n; j++) {
      double t = B[i][j];
      for (k = 0; k < j; k++) t -= Lc[j][k] * B[i][k];
      B[i][j] = t / Lc[j][j];
    }
  for (i = 0; i < n; i++) for (j = 0; j < n; j++) Q[i][j] = (i == j);
  for (i = 0; i < n; i++) for (j = i + 1; j < n; j++) B[i][j] = B[j][i] = 0.5 * (B[i][j] + B[j][i]);
  for (sweep = 0; sweep < 60; sweep++) {
    double off = 0.0, all = 0.0;
    int p, q;
    for (i = 0; i < n; i++) for (j = 0; j < n; j++) { all += B[i][j] * B[i][j]; if (i != j) off += B[i][j] * B[i][j]; }
    if (!isfinite(all)) return -1;
    if (off <= 1.0e-32 * all) break;
    for (p = 0; p < n - 1; p++) for (q = p + 1; q < n; q++) {
      const double apq = B[p][q];
      if (apq == 0.0) continue;
      const double tau = (B[q][q] - B[p][p]) / (2.0 * apq), t = (tau >= 0.0 ? 1.0 : -1.0) / (fabs(tau) + sqrt(1.0 + tau * tau));
      const double c = 1.0 / sqrt(1.0 + t * t), s = t * c;
      for (k = 0; k < n; k++) if (k != p && k != q) {
        const double bkp = B[k][p], bkq = B[k][q];
        B[k][p] = B[p][k] = c * bkp - s * bkq;
        B[k][q] = B[q][k] = s * bkp + c * bkq;
      }
      B[p][p] -= t * apq; B[q][q] += t * apq; B[p][q] = B[q][p] = 0.0;
      for (k = 0; k < n; k++) {
        const double qkp = Q[k][p], qkq = Q[k][q];
        Q[k][p] = c * qkp - s * qkq;
        Q[k][q] = s * qkp + c * qkq;
      }
    }
  }
  for (i = 0; i < n; i++) { if (!isfinite(B[i][i])) return -1; order[i] = i; }
  for (i = 1; i < n; i++) {                                        /* ascending, ties in index order */
    const int o = order[i];
    for (j = i; j > 0 && B[order[j - 1]][order[j - 1]] > B[o][o]; j--) order[j] = order[j - 1];
    order[j] = o;
  }
  for (j = 0; j < take; j++) {                                     /* C = D L^-T Q: back substitution */
    const int q = order[j];
    for (i = n - 1; i >= 0; i--) {
      double t = Q[i][q];
      for (k = i + 1; k < n; k++) t -= Lc[k][i] * y[k];
      y[i] = t / Lc[i][i];
    }
    for (i = 0; i < n; i++) { if (!isfinite(y[i])) return -1; }
    for (i = 0; i < n; i++) C[i * take + j] = d[i] * y[i];
    theta[j] = B[q][q];
  }
  return 0;
}

/* the default start block, column j, into an (N,N,N) host array: a product of low-order polynomials in the cell centre's coordinates about the middle of
 * the domain plus a quarter of a counter-based hash (splitmix64's finaliser) of the global cell index: a function of (N, j) only */
static void eig_default_start(int n, int j, double *v) {
  static const int px[EIG_M] = { 0, 1, 0, 0, 1, 1, 0, 2, 0, 0, 1, 2 }, py[EIG_M] = { 0, 0, 1, 0, 1, 0, 1, 0, 2, 0, 1, 1 }, pz[EIG_M] = { 0, 0, 0, 1, 0, 1, 1, 0, 0, 2, 1, 0 };
  int k;
#pragma omp parallel for
  for (k = 0; k < n; k++) for (int jj = 0; jj < n; jj++) for (int i = 0; i < n; i++) {      /* a cell's value depends on (n, j, cell) only: any thread gives it the same bits */
    int e;
    const double x = (i + 0.5) / n - 0.5, y = (jj + 0.5) / n - 0.5, z = (k + 0.5) / n - 0.5;
    const size_t cell = (size_t)i + (size_t)n * ((size_t)jj + (size_t)n * (size_t)k);
    unsigned long long t = (unsigned long long)cell + (unsigned long long)n * n * n * (unsigned long long)(j + 1);
    double poly = 1.0;
    t += 0x9e3779b97f4a7c15ULL; t ^= t >> 30; t *= 0xbf58476d1ce4e5b9ULL; t ^= t >> 27; t *= 0x94d049bb133111ebULL; t ^= t >> 31;
    for (e = 0; e < px[j]; e++) poly *= 2.0 * x;
    for (e = 0; e < py[j]; e++) poly *= 2.0 * y;
    for (e = 0; e < pz[j]; e++) poly *= 2.0 * z;
    v[cell] = poly + 0.25 * ((double)(t >> 11) * (1.0 / 9007199254740992.0) - 0.5);
  }
}

int hpgmg_user_eigs(hpgmg_user_solver *us, int k, int extra, double rtol, int max_iter, const double *x0, int where, double *lam, double *modes,
                    hpgmg_user_eig_info *info) {
  if (!us || !lam || !modes || (where != HPGMG_WHERE_HOST && where != HPGMG_WHERE_PLUGIN)) return HPGMG_USER_BAD_ARGUMENT;
  hpgmg_solver *s = &us->s;
  level_type *L = &s->level_h;
  mg_type *G = &s->mg;
  const int m = k + extra, helmholtz = s->a != 0.0, w_id = helmholtz ? VECTOR_ALPHA : -1;
  const size_t cells = (size_t)us->n * us->n * us->n;
  if (k < 1 || extra < 0 || m > EIG_M || (size_t)m > cells || !(rtol > 0.0) || max_iter < 0) return HPGMG_USER_BAD_ARGUMENT;
  if (!us->operator_ok) return HPGMG_USER_NOT_READY;
  if (!user_config_ok()) return HPGMG_USER_CONFLICT;
  if (L->must_subtract_mean == 1) return HPGMG_USER_UNSUPPORTED;       /* a singular operator: the V-cycle is no preconditioner for it without a deflation */
  USER_QUIET(us);
  if (helmholtz) {                                                    /* M = diag(alpha) must be positive definite: 1 / alpha is finite everywhere */
    invert_vector(L, VECTOR_TEMP, 1.0, VECTOR_ALPHA);
    if (!isfinite(norm(L, VECTOR_TEMP))) { USER_LOUD(); return HPGMG_USER_OUT_OF_RANGE; }
  }
  const double a = s->a, b = s->b;
  const int z_id = hpgmg_vectors_reserved() + 2;                       /* the CG solves' z: the V-cycle's correction must be a vector of every level */
  int X[EIG_M], AX[EIG_M], W[EIG_M], AW[EIG_M], P[EIG_M], AP[EIG_M], locked[EIG_M], act[EIG_M];
  int S[EIG_S], AS[EIG_S], l, j, q, na, np, have_p = 0, iterations = 0, vcycles = 0, broke = 0, st = HPGMG_USER_OK;
  double mu[EIG_M], rmax[EIG_M], mxmax[EIG_M], res[EIG_M];
  eig_work *work = (eig_work *)malloc(sizeof(eig_work));
  if (!work) { USER_LOUD(); return HPGMG_USER_BAD_ARGUMENT; }
  double *GA = work->GA, *GM = work->GM, *GA0 = work->GA0, *GM0 = work->GM0, *C = work->C, *C2 = work->C2;
  for (l = 0; l < G->num_levels; l++) create_vectors(G->levels[l], hpgmg_vectors_reserved() + 3);      /* allocates the first time only */
  if (us->eig_n < 6 * m) {                                             /* the block's vectors, on the finest level only */
    const int base = L->numVectors, more = 6 * m - us->eig_n;
    create_vectors(L, base + more);
    for (q = 0; q < more; q++) us->eig_ids[us->eig_n++] = base + q;
  }
  for (j = 0; j < m; j++) {
    X[j] = us->eig_ids[6 * j]; AX[j] = us->eig_ids[6 * j + 1]; W[j] = us->eig_ids[6 * j + 2]; AW[j] = us->eig_ids[6 * j + 3];
    P[j] = us->eig_ids[6 * j + 4]; AP[j] = us->eig_ids[6 * j + 5];
    locked[j] = 0;
  }
  /* the start block.  Nothing of the solver's state has been touched so far: a refused x0 leaves it as it was */
  if (x0) {
    for (j = 0; j < m && st == HPGMG_USER_OK; j++)
      st = user_pack_status(hpgmg_dense_pack(L, X[j], x0 + (size_t)j * cells, where, HPGMG_DENSE_CELL, HPGMG_DENSE_CHECK_FINITE));
  } else {
    double *v = (double *)malloc(cells * sizeof(double));
    for (j = 0; j < m; j++) { eig_default_start(us->n, j, v); hpgmg_dense_pack(L, X[j], v, HPGMG_WHERE_HOST, HPGMG_DENSE_CELL, HPGMG_DENSE_CHECK_FINITE); }
    free(v);
  }
  if (st != HPGMG_USER_OK) { free(work); USER_LOUD(); return st; }
  us->march = 0;
  us->rhs_ok = 0;                                                      /* the V-cycles and the applies use the solve's work vectors */
  MGPreconditionerBegin(G, 0, z_id, VECTOR_R, a, b);
  /* Rayleigh-Ritz on the start block: X becomes M-orthonormal with Ritz values mu */
  for (j = 0; j < m; j++) apply_op(L, AX[j], X[j], a, b);
  hpgmg_block_gram(L, X, m, AX, m, -1, GA);
  hpgmg_block_gram(L, X, m, X, m, w_id, GM);
  if (eig_ritz(work, m, GA, GM, m, C, mu) != 0) broke = 1;                   /* a dependent (or zero) start block */
  else { hpgmg_block_combine(L, X, m, X, m, C); hpgmg_block_combine(L, AX, m, AX, m, C); }
  while (!broke) {
    /* 1. residuals of every column into AW (which step 3 overwrites column by column) */
    int wanted = 0, n;
    hpgmg_block_residual(L, AW, AX, X, m, w_id, mu, rmax, mxmax);
    for (j = 0; j < m; j++) res[j] = rmax[j] / (mu[j] * mxmax[j]);
    /* 2. locking: a wanted column below rtol is done for good; the guards stay while a wanted one is active */
    for (j = 0; j < k; j++) { if (res[j] < rtol) locked[j] = 1; if (!locked[j]) wanted++; }
    if (!wanted || iterations >= max_iter) break;
    iterations++;
    for (na = 0, j = 0; j < m; j++) if (!locked[j]) act[na++] = j;
    /* 3. W_j = M^-1 R_j by one V-cycle, AW_j = A W_j */
    for (q = 0; q < na; q++) {
      j = act[q];
      scale_vector(L, VECTOR_R, 1.0, AW[j]);
      MGPreconditionerApply(G, 0, z_id, VECTOR_R, a, b);
      vcycles++;
      scale_vector(L, W[j], 1.0, z_id);
      apply_op(L, AW[j], W[j], a, b);
    }
    /* 4. the Gram matrices of S = [X, W_active, P_active] */
    for (n = 0, j = 0; j < m; j++, n++) { S[n] = X[j]; AS[n] = AX[j]; }
    for (q = 0; q < na; q++, n++) { S[n] = W[act[q]]; AS[n] = AW[act[q]]; }
    np = have_p ? na : 0;                  /* the columns active now were all active last time, so each has its P; a column locked since then leaves its P out */
    for (q = 0; q < np; q++, n++) { S[n] = P[act[q]]; AS[n] = AP[act[q]]; }
    hpgmg_block_gram(L, S, n, AS, n, -1, GA0);
    hpgmg_block_gram(L, S, n, S, n, w_id, GM0);
    /* 5. Rayleigh-Ritz; without P if the basis with it is dependent */
    memcpy(GA, GA0, sizeof(double) * n * n); memcpy(GM, GM0, sizeof(double) * n * n);
    if (eig_ritz(work, n, GA, GM, m, C, mu) != 0) {
      const int n2 = m + na;
      int r, c;
      for (r = 0; r < n2; r++) for (c = 0; c < n2; c++) { GA[r * n2 + c] = GA0[r * n + c]; GM[r * n2 + c] = GM0[r * n + c]; }
      np = 0; n = n2;
      if (eig_ritz(work, n, GA, GM, m, C, mu) != 0) { broke = 1; break; }
    }
    /* 6. X' = S C and A X' = (A S) C; P' = [W, P] C_WP and A P' likewise, for the active columns (a locked one never needs its P again) */
    hpgmg_block_combine(L, X, m, S, n, C);
    hpgmg_block_combine(L, AX, m, AS, n, C);
    {
      int Pout[EIG_M], APout[EIG_M], r;
      for (q = 0; q < na; q++) { Pout[q] = P[act[q]]; APout[q] = AP[act[q]]; }
      for (r = m; r < n; r++) for (q = 0; q < na; q++) C2[(r - m) * na + q] = C[r * m + act[q]];
      hpgmg_block_combine(L, Pout, na, S + m, n - m, C2);
      hpgmg_block_combine(L, APout, na, AS + m, n - m, C2);
      have_p = 1;
    }
    if (iterations % EIG_REFRESH == 0) for (j = 0; j < m; j++) apply_op(L, AX[j], X[j], a, b);
  }
  /* the final pass: one more Rayleigh-Ritz on X alone (it orders the pairs and makes h^3 X^T M X = I), A X applied afresh, mu the Rayleigh quotients of
   * the block returned and the residuals true ones */
  {
    const double scale = 1.0 / sqrt(L->h * L->h * L->h);
    int ok;
    hpgmg_block_gram(L, X, m, AX, m, -1, GA);
    hpgmg_block_gram(L, X, m, X, m, w_id, GM);
    memcpy(GM0, GM, sizeof(double) * m * m);
    ok = eig_ritz(work, m, GA, GM, m, C, mu) == 0;
    if (!ok) {                                                          /* keep the columns, normalise each where it has a norm */
      for (q = 0; q < m * m; q++) C[q] = 0.0;
      for (j = 0; j < m; j++) C[j * m + j] = (GM0[j * m + j] > 0.0 && isfinite(GM0[j * m + j])) ? 1.0 / sqrt(GM0[j * m + j]) : 1.0;
    }
    for (q = 0; q < m * m; q++) C[q] *= scale;
    hpgmg_block_combine(L, X, m, X, m, C);
    for (j = 0; j < m; j++) apply_op(L, AX[j], X[j], a, b);
    hpgmg_block_gram(L, X, m, AX, m, -1, GA);
    hpgmg_block_gram(L, X, m, X, m, w_id, GM);
    for (j = 0; j < m; j++) mu[j] = GA[j * m + j] / GM[j * m + j];
    hpgmg_block_residual(L, AW, AX, X, m, w_id, mu, rmax, mxmax);
    for (j = 0; j < m; j++) res[j] = rmax[j] / (mu[j] * mxmax[j]);
  }
  /* the k lowest of the m Rayleigh quotients, ascending (within a cluster they may have swapped against the Ritz values' order by a rounding) */
  int order[EIG_M];
  for (j = 0; j < m; j++) order[j] = j;
  for (j = 1; j < m; j++) {
    const int o = order[j];
    for (q = j; q > 0 && mu[order[q - 1]] > mu[o]; q--) order[q] = order[q - 1];
    order[q] = o;
  }
  for (j = 0; j < k && st == HPGMG_USER_OK; j++) if (hpgmg_dense_unpack(L, X[order[j]], modes + (size_t)j * cells, where) < 0) st = HPGMG_USER_BAD_ARGUMENT;
  free(work);
  USER_LOUD();
  if (st != HPGMG_USER_OK) return st;
  for (j = 0; j < k; j++) lam[j] = mu[order[j]] - a;
  if (info) {
    memset(info, 0, sizeof(*info));
    info->iterations = iterations; info->vcycles = vcycles;
    info->converged = !broke;
    for (j = 0; j < k; j++) {
      info->residuals[j] = res[order[j]]; info->mu[j] = mu[order[j]];
      if (!(res[order[j]] < rtol)) info->converged = 0;
    }
  }
  return HPGMG_USER_OK;
}
