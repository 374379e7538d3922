/*
 * hpgmg_boundary_math.h -- INTERNAL: the arithmetic of the dense-array boundary hooks (include/hpgmg_operators.h hpgmg_dense_*, hpgmg_boundary_*;
 * DESIGN.md §11.1, §11.2, §11.5, §11.6), written once for the host defaults (host/hooks_host.inc), the HIP plugin (host/plugin_dense.c) and its kernels
 * (kernels/dense_boundary.hip, kernels/dense_flux.hip, kernels/dense_sensitivity.hip, kernels/dense_cells.hip).  Not part of the C ABI: it declares nothing extern and no caller of the library includes it.
 *
 * The GPU tests hold the HIP build to the host defaults bit for bit, and every build has -ffp-contract=off, so the written order of each
 * floating-point expression here IS the contract: change one and both sides change together.  Whatever reads a vector of the level (the coarse
 * iterate, a beta) stays with the caller, which knows where that lives.
 *
 * Compiles as gnu99 C and as HIP C++.  Indices into a boundary array are int on both sides: 24 n^2 (the finer array under a lift) stays below
 * 2^31 up to n = 9459 cells per side, where one vector of the level would hold 6.7 TB.
 */
#ifndef HPGMG_BOUNDARY_MATH_H
#define HPGMG_BOUNDARY_MATH_H

#ifdef __HIPCC__
#define HPGMG_BND_FN __host__ __device__ __forceinline__
#else
#define HPGMG_BND_FN static inline
#endif

/* extent along one axis of a dense array of a level with n cells there; high_face: it is a face array of that axis on a Dirichlet level, which
 * holds the high domain face too */
HPGMG_BND_FN int dense_extent(int n, int high_face) { return n + (high_face != 0); }

/* A boundary array is 6 x n x n doubles (n cells per side, a cube): [0], [1] i-low / i-high indexed [k][j], [2], [3] j-low / j-high [k][i],
 * [4], [5] k-low / k-high [j][i]. */
HPGMG_BND_FN int bnd_touches(int n, int face, int gi, int gj, int gk) {          /* cell (gi,gj,gk) lies on domain face `face` */
  const int c = face < 2 ? gi : face < 4 ? gj : gk;
  return (face & 1) ? c == n - 1 : c == 0;
}
HPGMG_BND_FN int bnd_entry(int n, int face, int gi, int gj, int gk) {            /* its entry in the boundary array */
  const int q = face < 4 ? gk : gj, p = face < 2 ? gj : gi;
  return (face * n + q) * n + p;
}
/* BND_AT(face, i, j, k): the entry of `face` at the in-range cell (i, j, k) (its own axis not read) of the array g of an n-cube in scope */
#define BND_IDX(f, i, j, k) (((f) * n + ((f) < 4 ? (k) : (j))) * n + ((f) < 2 ? (j) : (i)))
#define BND_AT(f, i, j, k) g[BND_IDX(f, i, j, k)]

/* a Dirichlet face's entry of the lift is (w * beta) * g, a Neumann wall's (wn * wall beta) * gn (b the operator's b, h the level's h) */
HPGMG_BND_FN double bnd_weight(double b, double h) { return (2.0 * b) * (1.0 / (h * h)); }
HPGMG_BND_FN double bnd_weight_neumann(double b, double h) { return b * (1.0 / h); }
/* A Robin wall du/dn + kappa u = g, t = kappa * h of the level: the level's beta on the wall is wall * (t / (2.0 + t)), under
 * the kernels' Dirichlet wall term, and the wall's entry of the lift ((wn * wall) * g) * (2.0 / (2.0 + t)).  kappa = 0.0 is the Neumann wall bit
 * for bit: +0.0, and a last factor of exactly 1.0. */
HPGMG_BND_FN double bnd_wall_beta(double wall, double kappa, double h) { const double t = kappa * h; return wall * (t / (2.0 + t)); }
HPGMG_BND_FN double bnd_wall_phi(double wn, double wall, double g, double kappa, double h) { const double t = kappa * h; return ((wn * wall) * g) * (2.0 / (2.0 + t)); }
/* hpgmg_boundary_check_kappa's bits for entry e of a kappa array of an n-cube (robin_mask: bit f = face f is a Robin wall): the status bits
 * of hpgmg_dense_pack (1 not finite, anywhere; 2 negative on a Robin face), and BND_KAPPA_POSITIVE: > 0 on a Robin face */
#define BND_KAPPA_POSITIVE 4
HPGMG_BND_FN int bnd_kappa_bits(int n, int robin_mask, int e, double v) {
  if (!(v - v == 0.0)) return 1;
  if (!((robin_mask >> (e / (n * n))) & 1)) return 0;
  return v < 0.0 ? 2 : v > 0.0 ? BND_KAPPA_POSITIVE : 0;
}

/* Face fluxes of a solution (hpgmg_dense_unpack_flux): q = -b beta du/dx_d on a face of axis d, positive towards increasing
 * index, wq = bnd_weight_neumann(b, h).  Between two cells (a periodic wrap included) it is bnd_flux_interior.  On a Dirichlet wall the ghost is
 * 2 g - u_c and beta the level's; `high`: the wall is the high one of its axis.  On a masked wall (Neumann or Robin; wall, kappa the entries of
 * the solver's arrays, t = kappa * h) the OUTWARD flux is Q = ((b * wall) * (2.0 / (2.0 + t))) * (kappa * u_c - g): q = Q on a high wall, -Q on
 * a low one.  kappa = 0.0 is the Neumann wall bit for bit: a factor of exactly 1.0 and +-0.0 - g. */
HPGMG_BND_FN double bnd_flux_interior(double wq, double beta, double u_lo, double u_hi) { return (wq * beta) * (u_lo - u_hi); }
HPGMG_BND_FN double bnd_flux_dirichlet(double wq, double beta, double u_c, double g, int high) {
  return high ? (wq * beta) * (2.0 * (u_c - g)) : (wq * beta) * (2.0 * (g - u_c));
}
HPGMG_BND_FN double bnd_flux_masked(double b, double wall, double kappa, double h, double u_c, double g, int high) {
  const double t = kappa * h;
  const double Q = ((b * wall) * (2.0 / (2.0 + t))) * (kappa * u_c - g);
  return high ? Q : -Q;
}

/* Coefficient sensitivities (hpgmg_dense_unpack_sensitivity): G_p = d/dp sum_c lam_c (A0 u - T(g))_c for every coefficient entry p,
 * the bilinear twin of the fluxes above.  None reads a beta: the operator is affine in each.  w2 = bnd_sens_weight(b, h), w = bnd_weight(b, h),
 * wn = bnd_weight_neumann(b, h), t = kappa * h.
 *   alpha of cell c:                              a * (u_c * l_c)
 *   a face between two cells (the wrap included): w2 * ((u_lo - u_hi) * (l_lo - l_hi))
 *   a Dirichlet wall face of cell c, either side: (w * (u_c - g)) * l_c
 *   a masked wall face of cell c, either side:    ((wn * (2.0 / (2.0 + t))) * (kappa * u_c - g)) * l_c      (the wall's own beta)
 * The first two are symmetric in u and lam bit for bit: the product of the two states (of their differences) is formed first.  kappa = 0.0 is the
 * Neumann wall bit for bit: a factor wn * 1.0 and +-0.0 - g. */
HPGMG_BND_FN double bnd_sens_weight(double b, double h) { return b * (1.0 / (h * h)); }
HPGMG_BND_FN double bnd_sens_alpha(double a, double u_c, double l_c) { return a * (u_c * l_c); }
HPGMG_BND_FN double bnd_sens_interior(double w2, double u_lo, double u_hi, double l_lo, double l_hi) { return w2 * ((u_lo - u_hi) * (l_lo - l_hi)); }
HPGMG_BND_FN double bnd_sens_dirichlet(double w, double u_c, double g, double l_c) { return (w * (u_c - g)) * l_c; }
HPGMG_BND_FN double bnd_sens_masked(double wn, double kappa, double h, double u_c, double g, double l_c) {
  const double t = kappa * h;
  return ((wn * (2.0 / (2.0 + t))) * (kappa * u_c - g)) * l_c;
}

/* Cell-centred conductivities (hpgmg_dense_pack_cell_mean, hpgmg_dense_unpack_cell_sensitivity): the beta of a face between two
 * cells (box-to-box and the periodic wrap included) is a mean of the two, lo the cell with the smaller index along the axis (the wrap: lo = cell
 * N - 1, hi = cell 0); a domain wall face of any kind takes its cell's own value, derivative 1.0.  mean: HPGMG_MEAN_HARMONIC (0) or
 * HPGMG_MEAN_ARITHMETIC (1) of include/hpgmg_operators.h, which a caller has validated.
 *   bnd_mean:      harmonic (2.0 * (lo * hi)) / (lo + hi);  arithmetic 0.5 * (lo + hi)
 *   bnd_mean_dlo:  d/dlo: harmonic t = hi / (lo + hi), 2.0 * (t * t);  arithmetic 0.5
 *   bnd_mean_dhi:  d/dhi = bnd_mean_dlo with the two exchanged
 * bnd_cell_bits: the status bits of one k entry (1 not finite, 2 finite and not > 0: hpgmg_dense_pack's under CHECK_POSITIVE).  bnd_mean_bits: of a
 * mean whose two cells both passed: overflow of lo * hi or lo + hi gives 1, underflow to zero 2. */
HPGMG_BND_FN double bnd_mean(int mean, double lo, double hi) { return mean ? 0.5 * (lo + hi) : (2.0 * (lo * hi)) / (lo + hi); }
HPGMG_BND_FN double bnd_mean_dlo(int mean, double lo, double hi) {
  if (mean) return 0.5;
  const double t = hi / (lo + hi);
  return 2.0 * (t * t);
}
HPGMG_BND_FN double bnd_mean_dhi(int mean, double lo, double hi) { return bnd_mean_dlo(mean, hi, lo); }
HPGMG_BND_FN int bnd_cell_bits(double v) { return !(v - v == 0.0) ? 1 : !(v > 0.0) ? 2 : 0; }
HPGMG_BND_FN int bnd_mean_bits(double lo, double hi, double m) { return (bnd_cell_bits(lo) | bnd_cell_bits(hi)) ? 0 : bnd_cell_bits(m); }

/* S(c) of hpgmg_boundary_lift: the four finer entries under each face entry of coarse cell (gi,gj,gk) of an n-cube, faces in order */
HPGMG_BND_FN double bnd_fine_sum(int n, const double *phi_f, int gi, int gj, int gk) {
  const int nf = 2 * n;
  double S = 0.0;
  int face;
  for (face = 0; face < 6; face++) if (bnd_touches(n, face, gi, gj, gk)) {
    const int q = face < 4 ? gk : gj, p = face < 2 ? gj : gi;
    const double *e = phi_f + (face * nf + 2 * q) * nf + 2 * p;
    S = S + (((e[0] + e[1]) + e[nf]) + e[nf + 1]);
  }
  return S;
}

/* delta of the ghost at coarse (ci,cj,ck) between Dirichlet walls (hpgmg_boundary_interp): 2 g on a face, the wall-by-wall
 * linear rule on an edge or corner (exact for u linear near them) */
HPGMG_BND_FN double bnd_ghost_delta(int n, const double *g, int ci, int cj, int ck) {
  const int q[3] = { ci, cj, ck };
  int out[3], P[3], step[3], face[3], a, m = 0;
  for (a = 0; a < 3; a++) {
    out[a] = q[a] < 0 || q[a] >= n;
    P[a] = q[a] < 0 ? 0 : q[a] >= n ? n - 1 : q[a];
    step[a] = q[a] < 0 ? 1 : -1;                               /* one cell inward */
    face[a] = 2 * a + (q[a] >= n);
    m += out[a];
  }
  if (m == 1) { a = out[0] ? 0 : out[1] ? 1 : 2; return 2.0 * BND_AT(face[a], P[0], P[1], P[2]); }
  if (n < 2) return m == 3 ? ((BND_AT(face[0], P[0], P[1], P[2]) + BND_AT(face[1], P[0], P[1], P[2])) + BND_AT(face[2], P[0], P[1], P[2])) * (2.0 / 3.0) : 0.0;
  if (m == 2) {                      /* the outside axes x < y: each wall's entry next to the edge minus the one a cell further along the other wall */
    const int x = out[0] ? 0 : 1, y = out[2] ? 2 : 1;
    const int yi = P[0] + (y == 0) * step[0], yj = P[1] + (y == 1) * step[1], yk = P[2] + (y == 2) * step[2];
    const int xi = P[0] + (x == 0) * step[0], xj = P[1] + (x == 1) * step[1], xk = P[2] + (x == 2) * step[2];
    return (BND_AT(face[x], P[0], P[1], P[2]) - BND_AT(face[x], yi, yj, yk)) + (BND_AT(face[y], P[0], P[1], P[2]) - BND_AT(face[y], xi, xj, xk));
  }
  double c[3];                       /* corner: each wall's linear extrapolation to the corner point */
  for (a = 0; a < 3; a++) {
    const int b = a == 0 ? 1 : 0, d = a == 2 ? 1 : 2;          /* the wall's in-face axes, b < d */
    const double g00 = BND_AT(face[a], P[0], P[1], P[2]);
    const double g10 = BND_AT(face[a], P[0] + (b == 0) * step[0], P[1] + (b == 1) * step[1], P[2]);
    const double g01 = BND_AT(face[a], P[0], P[1] + (d == 1) * step[1], P[2] + (d == 2) * step[2]);
    c[a] = (2.0 * g00 - 0.5 * g10) - 0.5 * g01;
  }
  return ((c[0] + c[1]) + c[2]) * (2.0 / 3.0);
}

/* The same ghost with per-face kinds (hpgmg_boundary_interp_faces / _robin; bit f of mask: face f is a Neumann or Robin
 * wall, hc the coarse h, kappa the coarse level's kappa array, NULL: every masked wall is Neumann).
 * Its delta is  needs_u ? c * u + s : s  with u the coarse iterate at the in-range cell P, which the caller reads.  Between Dirichlet walls
 * alone (any ghost under mask 0) needs_u is 0 and s is bnd_ghost_delta: no 0 * u + s, which would turn an s of -0.0 into +0.0.
 * Else, m the number of outside axes: c = (1 - (-1)^m) + per outside axis in the order i, j, k (k_a - 1.0), s = 0.0 + per outside axis s_a, with
 * Dirichlet k_a - 1.0 = -2.0, s_a = 2.0 * g;  Neumann 0, hc * gn;  Robin, t = kappa * hc: (2.0 - t) / (2.0 + t) - 1.0, (2.0 * hc / (2.0 + t)) * g.
 * Without a Robin wall c is a small integer however it is summed (the bits of §11.2's 1 - 2 * dirichlet -+ 1), and kappa = 0.0 gives Neumann's
 * terms bit for bit: 2.0 / 2.0 - 1.0 and (2.0 * hc / 2.0) * g. */
typedef struct { int needs_u, P[3]; double c, s; } bnd_ghost;
HPGMG_BND_FN bnd_ghost bnd_ghost_faces(int n, const double *g, double hc, int mask, const double *kappa, int ci, int cj, int ck) {
  const int q[3] = { ci, cj, ck };
  int out[3], face[3], a, m = 0, dirichlet = 0;
  bnd_ghost G;
  for (a = 0; a < 3; a++) {
    out[a] = q[a] < 0 || q[a] >= n;
    G.P[a] = q[a] < 0 ? 0 : q[a] >= n ? n - 1 : q[a];
    face[a] = 2 * a + (q[a] >= n);
    m += out[a];
    dirichlet += out[a] && !((mask >> face[a]) & 1);
  }
  G.needs_u = dirichlet != m;
  G.c = 0.0;
  if (!G.needs_u) { G.s = bnd_ghost_delta(n, g, ci, cj, ck); return G; }
  double s = 0.0, c = (m & 1) ? 2.0 : 0.0;
  for (a = 0; a < 3; a++) if (out[a]) {
    const int e = BND_IDX(face[a], G.P[0], G.P[1], G.P[2]);
    const double ga = g[e];
    if (!((mask >> face[a]) & 1)) { c = c + -2.0; s = s + 2.0 * ga; }
    else if (!kappa) s = s + hc * ga;
    else {
      const double t = kappa[e] * hc;
      c = c + ((2.0 - t) / (2.0 + t) - 1.0);
      s = s + (2.0 * hc / (2.0 + t)) * ga;
    }
  }
  G.c = c;
  G.s = s;
  return G;
}
#undef BND_AT
#undef BND_IDX

/* D(c) of hpgmg_boundary_interp / _interp_faces for a fine cell is the sum over t = 1 .. 7, in this order, of w * delta for the reads of
 * interpolation_p1 after the centre (dk, dj, dj+dk, di, di+dk, di+dj, di+dj+dk) that are ghosts of the coarse nc-cube; delta is bnd_ghost_delta
 * of the ghost between Dirichlet walls, bnd_ghost_faces' with per-face kinds.  bnd_p1_of: the fine cell's coarse cell c and the side d it leans
 * to, once per cell.  bnd_p1_ghost: whether read t is a ghost, and then its coarse cell q and its p1 weight *w. */
typedef struct { int c[3], d[3]; } bnd_p1_cell;
HPGMG_BND_FN bnd_p1_cell bnd_p1_of(int gi, int gj, int gk) {
  const bnd_p1_cell F = { { gi >> 1, gj >> 1, gk >> 1 }, { (gi & 1) ? 1 : -1, (gj & 1) ? 1 : -1, (gk & 1) ? 1 : -1 } };
  return F;
}
HPGMG_BND_FN int bnd_p1_ghost(int nc, bnd_p1_cell F, int t, int q[3], double *w) {
  const double wt[8] = { 0.421875, 0.140625, 0.140625, 0.046875, 0.140625, 0.046875, 0.046875, 0.015625 };
  q[0] = F.c[0] + ((t >> 2) & 1) * F.d[0]; q[1] = F.c[1] + ((t >> 1) & 1) * F.d[1]; q[2] = F.c[2] + (t & 1) * F.d[2];
  *w = wt[t];
  return q[0] < 0 || q[0] >= nc || q[1] < 0 || q[1] >= nc || q[2] < 0 || q[2] >= nc;
}

#endif
